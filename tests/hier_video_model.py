"""A toy hierarchical net in numpy, run both ways over a video: the model behind tests/test_hier_video_host.py.

The real net's levels are per-frame functions (eval-mode BatchNorm, convs whose result does not depend on the batch) with a
join of three frames between them.  Here a frame is a small float32 vector, the cells of level L are an elementwise map that
differs from level to level (so that a level computed with another level's cells shows), and the join is either the max
in frame order or an order-sensitive three-tap filter in the library's pinned form.  `clip_path` is the reference: one
clip of T = 3^n frames per frame of the video (video.window_indices), pooled by consecutive triples as the clip net does.
`chunk_path` is the video path: video.hier_video_chunks' frame indices and counts, every join a dilated triple.  Both are
float32 throughout, so equality is bit for bit."""
import numpy as np

from videoyolo_amd import video

F32 = np.float32


def cells(level, x):
    """The per-frame cells of level `level` (0: the stem): nonlinear, different at every level, float32."""
    x = np.asarray(x, F32)
    a, b = F32(0.75 + 0.125 * level), F32(0.1 * (level + 1))
    y = (x * a + b).astype(F32)
    return np.where(y > 0, y, (y * F32(0.1)).astype(F32)).astype(F32)


def join_max(x0, x1, x2):
    """strict > in frame order: the earliest operand's bits on ties"""
    m = np.array(x0, F32, copy=True)
    for v in (x1, x2):
        m = np.where(v > m, v, m)
    return m.astype(F32)


W3 = (F32(0.5), F32(-1.25), F32(2.0))


def join_filter(x0, x1, x2):
    """fl32(w2 x2 + fl32(w1 x1 + fl32(w0 x0))) with three different weights: swapping two operands changes the result"""
    p0 = (W3[0] * np.asarray(x0, F32)).astype(F32)
    p1 = (p0 + (W3[1] * np.asarray(x1, F32)).astype(F32)).astype(F32)
    return (p1 + (W3[2] * np.asarray(x2, F32)).astype(F32)).astype(F32)


JOINS = {"max": join_max, "filter": join_filter}


def clip_path(frames, pools, step, join):
    """(N, D) video -> (N, D): level `pools` of the clip of every frame, as the clip net computes it"""
    frames = np.asarray(frames, F32)
    table = video.window_indices(len(frames), 3 ** pools, step)
    x = cells(0, frames[table])  # (N, T, D)
    for level in range(1, pools + 1):
        t = x.reshape(x.shape[0], -1, 3, x.shape[-1])
        x = cells(level, JOINS[join](t[:, :, 0], t[:, :, 1], t[:, :, 2]))
    assert x.shape[1] == 1
    return x[:, 0]


def chunk_path(frames, pools, step, frames_per_step, join):
    """The same through video.hier_video_chunks: per chunk the stem on the level-0 frames, then `pools` dilated joins, each
    on exactly the counts the function names; the padding of the last chunk is dropped"""
    frames = np.asarray(frames, F32)
    chunks, counts = video.hier_video_chunks(len(frames), pools, step, frames_per_step)
    out = []
    for centres, index in chunks:
        assert len(index) == counts[0]
        x = cells(0, frames[index])
        for level in range(1, pools + 1):
            d = step * 3 ** (level - 1)
            n = counts[level]
            assert len(x) == n + 2 * d == counts[level - 1]
            x = cells(level, JOINS[join](x[:n], x[d:d + n], x[2 * d:2 * d + n]))
        assert len(x) == frames_per_step
        out.append(x[:len(centres)])
    return np.concatenate(out, 0)
