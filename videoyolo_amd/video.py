"""A window net over a whole video: Darknet-53 once per frame.

The reference's windowed detect loop (``detect_yolo3.py --window k,step``) takes one k-frame clip per frame of the video
(``datasets/imgnetvid.py:480-506``): centred on the frame, ``step`` apart, clamped at the ends.  Consecutive clips share
frames, and with the early join a frame's three routes are the same bits in every clip, so a ``VideoSession`` runs the stem
and the stages once per frame, keeps the routes in a ring of slots inside its workspace and pools every clip out of the ring
(``vy_net_video_push`` / ``vy_net_video_detect``, include/vyolo.h).  The detections are bit-identical to
``net(frames[window_indices(T, k, step)])``.

``window_indices`` and ``RingSchedule`` are plain Python (no device): the table of the reference's loop, and the
frame -> slot bookkeeping a session follows.

A hierarchical net (``hier_detect_video(net, frames)``) needs no ring: ``hier_video_chunks`` (plain Python too) cuts the video into
stateless chunks of centres, each with the level-0 frames its levels reach, and ``hier_detect_video`` runs them on a
hier-video plan (``vy_net_bind_hier_video`` / ``vy_net_hier_video_detect``), every level once per frame position.
"""
import ctypes

import numpy as np

from . import _lib
from .model import _ptrs, _route_shapes


def window_indices(n_frames, k, step=1):
    """``(n_frames, k)`` int64: row i = the frames of the clip the reference builds for frame i (imgnetvid.py:486-506).
    With ``w = k // 2`` the offsets are ``-w*step, ..., 0, ..., +w*step``, an even k drops the last one, and every index is
    clamped to ``[0, n_frames - 1]``."""
    n_frames, k, step = int(n_frames), int(k), int(step)
    if n_frames < 1 or k < 1 or step < 1:
        raise ValueError("window_indices: n_frames, k and step must be >= 1 (got %d, %d, %d)" % (n_frames, k, step))
    off = (np.arange(k, dtype=np.int64) - k // 2) * step
    return np.clip(np.arange(n_frames, dtype=np.int64)[:, None] + off[None, :], 0, n_frames - 1)


def min_ring(k, step, frames_per_step):
    """Smallest safe ring: ``frames_per_step + (k - 1) * step`` slots.  A push stores up to ``frames_per_step`` new frames
    before the clips they complete are pooled; the oldest clip still pending then reaches ``(k // 2) * step`` frames back
    from its centre, which itself lies ``(k - 1 - k // 2) * step`` frames (the window's look-ahead) behind the first new
    frame.  Frame j lives in slot ``j % ring``, so all of these must be distinct slots."""
    return int(frames_per_step) + (int(k) - 1) * int(step)


def hier_reach(pools, step, level):
    """``h_L = step * (3^L - 1) / 2``: how far level L of a hierarchical net reaches on either side of its position."""
    return int(step) * (3 ** int(level) - 1) // 2


def hier_video_chunks(n_frames, pools, step=1, frames_per_step=16):
    """The chunks of ``hier_detect_video`` over a video of ``n_frames`` frames, for a net of ``pools`` pools (clips of
    ``T = 3 ** pools`` frames, ``step`` apart) run ``frames_per_step`` centres at a time -> ``(chunks, counts)``.

    ``chunks``: one ``(centres, frame_index)`` per call.  ``centres`` lists the frames the call emits, at most
    ``frames_per_step`` consecutive ones (fewer in the last chunk: the plan still runs ``frames_per_step`` centres, and the
    outputs behind ``len(centres)`` are dropped).  ``frame_index`` (int64, ``frames_per_step + 2 h_n`` entries) is the
    level-0 input: entry j is frame ``clamp(a - h_n + j, 0, n_frames - 1)``, a the first centre — all the clamping of
    ``window_indices(n_frames, T, step)`` lives here.
    ``counts``: per level L = 0 .. pools the positions a call holds of it, ``frames_per_step + 2 (h_n - h_L)``, level L
    starting at position ``a - (h_n - h_L)``; join L -> L + 1 is ``dst[p] = join(src[p], src[p + d], src[p + 2d])`` with
    ``d = step * 3 ** L``."""
    n_frames, pools, step, f = int(n_frames), int(pools), int(step), int(frames_per_step)
    if n_frames < 1 or not 1 <= pools <= 4 or f < 1 or f > _lib.VY_VIDEO_TABLE_MAX or not 1 <= step <= _lib.VY_HIER_VIDEO_STEP_MAX:
        raise ValueError("hier_video_chunks: n_frames >= 1, pools in 1..4, step in 1..%d, frames_per_step in 1..%d (got %d, %d, "
                         "%d, %d)" % (_lib.VY_HIER_VIDEO_STEP_MAX, _lib.VY_VIDEO_TABLE_MAX, n_frames, pools, step, f))
    reach = hier_reach(pools, step, pools)
    counts = [f + 2 * (reach - hier_reach(pools, step, level)) for level in range(pools + 1)]
    chunks = []
    for a in range(0, n_frames, f):
        index = np.clip(np.arange(a - reach, a + f + reach, dtype=np.int64), 0, n_frames - 1)
        chunks.append((list(range(a, min(a + f, n_frames))), index))
    return chunks, counts


def hier_detect_video(net, frames, step=1, frames_per_step=16, return_index=False):
    """``(ids, scores, bboxes)`` for the ``(N, 3, H, W)`` video ``frames`` (host array or device tensor, any N >= 1) on the
    hierarchical net ``net`` (``YOLOV3Hier`` or ``YOLOV3HierConv``), one row-block per frame: bit for bit
    ``net(frames[window_indices(N, T, step)])``, the clips of the reference's ``detect_yolo3.py --window T,step``, but with
    the stem and every group of cells run once per frame position instead of once per clip.  ``frames_per_step`` frames are
    emitted per library call, which recomputes the ``step * (T - 1) / 2`` frames of context on either side: nothing is kept
    between calls, the last chunk is padded and the padding dropped.  ``frames`` is only read; a host video is uploaded once
    per chunk's frame range.  The call takes the net's workspace binding; a later clip or training call binds its own plan
    again.  One rank only.  (A function, not a method: the public surface of the model classes is pinned.)"""
    from .model import YOLOV3Hier
    if not isinstance(net, YOLOV3Hier):
        raise TypeError("hier_detect_video takes a hierarchical net (YOLOV3Hier / YOLOV3HierConv), got %s" % type(net).__name__)
    import torch
    from . import parallel
    if parallel.world_size() > 1:
        raise NotImplementedError("video detection of a hierarchical net is not supported on more than one rank")
    shape = tuple(frames.shape) if hasattr(frames, "shape") else tuple(np.shape(frames))
    if len(shape) != 4 or shape[1] != 3 or shape[0] < 1:
        raise ValueError("expected (n, 3, H, W) frames with n >= 1, got %s" % (shape,))
    chunks, counts = hier_video_chunks(shape[0], net._pools, step, frames_per_step)
    net._need_device()
    on_device = isinstance(frames, torch.Tensor) and frames.device == torch.device(net._device)
    if not on_device and not isinstance(frames, torch.Tensor):
        frames = torch.as_tensor(np.asarray(frames, np.float32))
    f = int(frames_per_step)
    outs = []
    with torch.cuda.device(net._device):
        net._ensure_hier_video(f, int(step), shape[2], shape[3])
        for centres, index in chunks:
            lo, hi = int(index[0]), int(index[-1])
            # the frame range of the chunk: a view of a device video, one upload of a host one — never once per clip
            span = frames[lo:hi + 1].to(device=net._device, dtype=torch.float32)
            if len(index) == hi + 1 - lo and span.is_contiguous():
                x = span  # an interior chunk reads its frames in place
            else:  # clamped at an end of the video (or a strided input): the level-0 frames gathered, counts[0] of them
                x = span.index_select(0, torch.as_tensor(index - lo, device=span.device)).contiguous()
            assert x.shape[0] == counts[0]
            got = net._detect_call("vy_net_hier_video_detect", f, _ptrs([x]), return_index)
            outs.append(tuple(t[:len(centres)] for t in got))
    return tuple(torch.cat(ts, 0) for ts in zip(*outs))


class RingSchedule:
    """The bookkeeping of a session, without a device: which frame goes to which ring slot and which slots every clip
    reads.  ``push(n)`` and ``flush()`` return the library calls to make, in order, as tuples

        ("push", frame_ids, slots)   frame_ids: the c <= F new frames of this backbone call; slots: F entries, -1 = padding
        ("detect", frame_ids, table) frame_ids: the m <= B frames emitted by this call; table: (B, k) slots, rows >= m
                                     repeat row m - 1 (their output is dropped)
    """

    def __init__(self, k, step=1, frames_per_step=16, clips_per_step=None, ring=None):
        self.k, self.step, self.F = int(k), int(step), int(frames_per_step)
        if self.k < 2 or self.step < 1 or self.F < 1:
            raise ValueError("video schedule: k >= 2, step >= 1, frames_per_step >= 1 (got %d, %d, %d)"
                             % (self.k, self.step, self.F))
        if self.F > _lib.VY_VIDEO_TABLE_MAX:
            raise ValueError("frames_per_step %d: at most %d (the slot table travels in the kernel arguments)"
                             % (self.F, _lib.VY_VIDEO_TABLE_MAX))
        self.B = int(clips_per_step) if clips_per_step else min(self.F, _lib.VY_VIDEO_TABLE_MAX // self.k)
        if self.B < 1 or self.B * self.k > _lib.VY_VIDEO_TABLE_MAX:
            raise ValueError("clips_per_step %d x k %d: at most %d table entries" % (self.B, self.k, _lib.VY_VIDEO_TABLE_MAX))
        need = min_ring(self.k, self.step, self.F)
        self.R = need if ring is None else int(ring)
        if self.R < need:
            raise ValueError("ring of %d slots is too small: k = %d, step = %d, frames_per_step = %d need %d "
                             "(frames_per_step + (k - 1) * step)" % (self.R, self.k, self.step, self.F, need))
        self.ahead = (self.k - 1 - self.k // 2) * self.step  # frames a window reaches past its centre
        self.offsets = [(t - self.k // 2) * self.step for t in range(self.k)]
        self.reset()

    def reset(self):
        self.pushed = 0   # frames stored so far (frame j sits in slot j % R while it is among the last R)
        self.emitted = 0  # frames whose detections were returned

    def _detects(self, upto, last):
        """Detect calls for frames [emitted, upto), windows clamped to [0, last]."""
        ops = []
        while self.emitted < upto:
            ids = list(range(self.emitted, min(upto, self.emitted + self.B)))
            rows = [[min(max(i + o, 0), last) % self.R for o in self.offsets] for i in ids]
            rows += [rows[-1]] * (self.B - len(rows))
            ops.append(("detect", ids, rows))
            self.emitted = ids[-1] + 1
        return ops

    def push(self, n):
        ops = []
        n = int(n)
        while n > 0:
            c = min(n, self.F)
            ids = list(range(self.pushed, self.pushed + c))
            ops.append(("push", ids, [j % self.R for j in ids] + [-1] * (self.F - c)))
            self.pushed += c
            n -= c
            # every frame whose look-ahead is stored: no clamp at the far end can apply to these
            ops += self._detects(self.pushed - self.ahead, self.pushed - 1)
        return ops

    def flush(self):
        ops = self._detects(self.pushed, self.pushed - 1)
        self.reset()
        return ops


class VideoSession:
    """``net.video(...)``: the video plan of a window net, its workspace (ring included) and the frame -> slot
    bookkeeping.  ``push(frames)`` returns the detections of every frame whose window is now complete, ``flush()`` those of
    the remaining frames (windows clamped to the last frame pushed) and resets the session for the next video.

    The session takes the net's workspace binding.  A clip or training call on the net afterwards binds its own plan
    again; the session re-binds the video plan at its next use if it holds no frames, and raises otherwise: the ring's
    contents do not survive a re-bind.  One rank only, exact fp32 conv mode only, no graph capture."""

    def __init__(self, net, frames_per_step=16, step=1, ring=None, clips_per_step=None):
        from . import parallel
        if parallel.world_size() > 1:
            raise NotImplementedError("video detection of a window net is not supported on more than one rank")
        net._need_device()
        self._net = net
        self._sched = RingSchedule(net.k, step, frames_per_step, clips_per_step, ring)
        self._hw = None    # frame size of the bound plan
        self._ws = None    # torch uint8 workspace of the video plan
        self._xbuf = None  # (F, 3, H, W) staging for a chunk shorter than F
        self._take_binding()

    frames_per_step = property(lambda self: self._sched.F)
    clips_per_step = property(lambda self: self._sched.B)
    ring = property(lambda self: self._sched.R)
    step = property(lambda self: self._sched.step)

    # ------------------------------------------------------------------ binding
    def _take_binding(self):
        """The net's next clip / training call must bind its own plan again, and this session its own."""
        self._net._drop_plan()
        self._net._video = self
        self._bound = False

    def _ensure_bound(self, h, w):
        net, s = self._net, self._sched
        if net._video is not self:
            if s.pushed:
                s.reset()
                raise RuntimeError("the net was bound to another plan (a clip call, a training call or another session) while "
                                   "this session held frames: the ring is lost; the session was reset, push the video again")
            self._take_binding()
        if self._bound and self._hw == (h, w):
            return
        if s.pushed:
            raise ValueError("frame size changed from %s to %s inside a video: flush() first" % (self._hw, (h, w)))
        need = net._lib.vy_net_video_workspace_bytes(net._h, s.F, s.B, s.R, h, w)
        if self._ws is not None and self._ws.numel() < need:
            self._ws = None  # released before its successor is allocated
        self._ws = net._size_and_bind(self._ws, need, lambda ws, nbytes: net._lib.vy_net_bind_video(
            net._h, ws, nbytes, s.F, s.B, s.R, h, w, net._stream()))
        self._xbuf = None
        self._hw, self._bound = (h, w), True

    # ------------------------------------------------------------------ the two library calls and the taps
    def raw_push(self, x, slots):
        """``vy_net_video_push``: x (F, 3, H, W) on the device, slots F entries in [-1, ring)."""
        net = self._net
        arr = (ctypes.c_int32 * len(slots))(*[int(v) for v in slots])
        _lib.check(net._lib.vy_net_video_push(net._h, ctypes.c_void_p(x.data_ptr()), arr, net._stream()))

    def raw_detect(self, table, return_index=False):
        """``vy_net_video_detect``: table (B, k) slots; outputs at batch B."""
        net, b = self._net, self._sched.B
        flat = [int(v) for row in table for v in row]
        if len(flat) != b * net.k:
            raise ValueError("slot table of %d entries, expected %d x %d" % (len(flat), b, net.k))
        return net._detect_call("vy_net_video_detect", b, [(ctypes.c_int32 * len(flat))(*flat)], return_index)

    def slot_of(self, frame):
        """Ring slot that holds (or held) frame `frame` of the current video."""
        return int(frame) % self._sched.R

    def read_slot(self, slot):
        """Test tap (``vy_net_video_read_slot``): the three routes in `slot`, NCHW with batch 1 — what
        ``YOLOV3.extract_features`` gives for that frame."""
        import torch
        net = self._net
        h, w = self._hw
        outs = [torch.empty(shape, dtype=torch.float32, device=net._device) for shape in _route_shapes(1, h, w)]
        with torch.cuda.device(net._device):
            _lib.check(net._lib.vy_net_video_read_slot(net._h, int(slot), *_ptrs(outs), net._stream()))
        return tuple(outs)

    def read_activation(self, name):
        """``net.read_activation`` on the video plan (needs ``net.keep_activations()`` before the session is opened): a
        stage cell's tap has the F frames of the last push, ``pool.i`` and the head cells the B clips of the last detect."""
        return self._net._read_tap(name, self._sched.F if name.startswith("stages.") else self._sched.B)

    # ------------------------------------------------------------------ the session
    def _as_frames(self, frames):
        import torch
        net = self._net
        if not isinstance(frames, torch.Tensor):
            frames = torch.as_tensor(np.asarray(frames, np.float32))
        if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] < 1:
            raise ValueError("expected (n, 3, H, W) frames with n >= 1, got %s" % (tuple(frames.shape),))
        return frames.to(device=net._device, dtype=torch.float32).contiguous()

    def _run(self, ops, frames, first, return_index):
        """Execute schedule ops; `frames` holds the frames from index `first` of the video on."""
        import torch
        net, s = self._net, self._sched
        outs = []
        for op, ids, table in ops:
            if op == "push":
                x = frames[ids[0] - first: ids[-1] + 1 - first]
                if len(ids) < s.F:  # a short chunk: the library always runs its planned F frames
                    if self._xbuf is None:
                        self._xbuf = torch.zeros((s.F,) + tuple(x.shape[1:]), dtype=torch.float32, device=net._device)
                    self._xbuf[:len(ids)].copy_(x)
                    x = self._xbuf
                self.raw_push(x, table)
            else:
                got = self.raw_detect(table, return_index=return_index)
                outs.append(tuple(t[:len(ids)] for t in got))
        return outs

    def _join(self, outs, return_index):
        import torch
        net = self._net
        if outs:
            return tuple(torch.cat(ts, 0) for ts in zip(*outs))
        outs = net._detect_outputs(0, net._out_rows() if self._bound else 0, return_index)
        return outs if return_index else outs[:3]

    def push(self, frames, return_index=False):
        """Store ``frames`` ((n, 3, H, W), host or device, n >= 1) and return ``(ids, scores, bboxes)`` of every frame whose
        window is now complete: one row-block per frame, in frame order — possibly none (leading dimension 0)."""
        import torch
        frames = self._as_frames(frames)
        with torch.cuda.device(self._net._device):
            self._ensure_bound(int(frames.shape[2]), int(frames.shape[3]))
            first = self._sched.pushed
            return self._join(self._run(self._sched.push(frames.shape[0]), frames, first, return_index), return_index)

    def flush(self, return_index=False):
        """Detections of the frames not yet returned, their windows clamped to the last frame pushed; the session is then
        empty and takes the next video (any frame size)."""
        import torch
        with torch.cuda.device(self._net._device):
            if self._sched.pushed:
                self._ensure_bound(*self._hw)
            return self._join(self._run(self._sched.flush(), None, 0, return_index), return_index)


def detect_video_features(net, f1, f2, f3, step=1, clips_per_step=16, return_index=False):
    """``YOLOV3NoBackboneWindow.detect_video_features``: every frame of a stored video from its ``(T, C, h, w)`` routes.  The
    clips are ``window_indices(T, k, step)``, ``clips_per_step`` rows per call on one plan; the last chunk is padded by
    repeating its last row, whose output is dropped.  The banks go to the device once and are read in place."""
    import torch
    b = int(clips_per_step)
    if b < 1 or b * net.k > _lib.VY_VIDEO_TABLE_MAX:
        raise ValueError("clips_per_step %d x k %d: between 1 and %d table entries" % (b, net.k, _lib.VY_VIDEO_TABLE_MAX))
    shape = tuple(f1.shape) if hasattr(f1, "shape") else tuple(np.shape(f1))
    if len(shape) != 4 or shape[0] < 1:
        raise ValueError("expected (T, C, h, w) routes with T >= 1, got %s" % (shape,))
    table = window_indices(shape[0], net.k, step)
    if net._device is not None:
        f1, f2, f3 = (net._dev(f) for f in (f1, f2, f3))
    outs = []
    for i in range(0, len(table), b):
        rows = table[i:i + b]
        m = len(rows)
        if m < b:
            rows = np.concatenate([rows, np.repeat(rows[-1:], b - m, axis=0)], 0)
        got = net.from_bank(f1, f2, f3, rows, return_index=return_index)
        outs.append(tuple(t[:m] for t in got))
    return tuple(torch.cat(ts, 0) for ts in zip(*outs))
