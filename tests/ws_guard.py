"""Guard bands around and inside a workspace: the checker of tests/test_ws_guard_host.py and tests/test_gpu_ws_guard.py.

A net created under VY_PLAN_GUARD=<bytes> leaves that many unused bytes behind every region its plans carve
(vy_net_plan_region, include/vyolo.h).  Here: the region table of a plan (`regions`), a caller's buffer with a band on
either side of the bytes the library binds (`banded`), the fill of every byte no launch may touch — the gaps, the
rounding slack behind each region's used bytes, the bands — with one quiet-NaN pattern (`poison`), and the comparison
of a host copy with that pattern (`violations`).

The pattern is a quiet NaN whose payload no kernel of the library produces (the hardware's own NaNs are 0x7fc00000 and
0xffc00000, with the sign or a propagated payload at most): "still poison" is an exact comparison, and a poison word
that reaches a result shows there as NaN.  It is laid by absolute byte position — byte i of the buffer holds byte i % 4
of the word — so a region that ends between words is handled like any other.
"""
import ctypes

import numpy as np

from videoyolo_amd import _lib

POISON = 0x7FC5A5C3
POISON_BYTES = np.frombuffer(np.uint32(POISON).tobytes(), np.uint8)
BAND = 1 << 16
GUARD = 4096

PLANS = {"clip": _lib.VY_PLAN_CLIP, "train": _lib.VY_PLAN_TRAIN, "video": _lib.VY_PLAN_VIDEO}
SIZERS = {"clip": "vy_net_workspace_bytes", "train": "vy_net_train_workspace_bytes", "video": "vy_net_video_workspace_bytes"}


def plan_bytes(lib, handle, plan, shape):
    """The matching *_workspace_bytes.  shape: (batch, height, width); a video plan: (frames, clips, ring, height, width)"""
    return int(getattr(lib, SIZERS[plan])(handle, *shape))


def check_table(table, total, exact=True):
    """Offsets ascend, regions are 256-byte aligned and disjoint, every one has bytes in use, the last one ends at `total`
    (exact=False: at or before it — a plan bound in a buffer sized for a larger one)."""
    assert table, "an empty region table"
    end = 0
    for name, off, used, span in table:
        assert off % 256 == 0 and span % 256 == 0, (name, off, span)
        assert off >= end, "region %s at %d overlaps its predecessor, which ends at %d" % (name, off, end)
        assert 0 < used <= span, (name, used, span)
        end = off + span
    assert end == total or (not exact and end < total), "the table ends at %d, the plan at %d" % (end, total)
    assert len({t[0] for t in table}) == len(table), "two regions of one name"


def regions(lib, handle, plan, shape):
    """[(name, offset, used bytes, bytes up to the next region)] of a plan, checked (check_table) against its size query."""
    if plan == "video":
        frames, clips, ring, h, w = shape
        args = (clips, h, w, frames, ring)
    else:
        args = tuple(shape) + (0, 0)
    table, r = [], _lib.PlanRegion()
    while True:
        rc = lib.vy_net_plan_region(handle, PLANS[plan], *args, len(table), ctypes.byref(r))
        if rc == _lib.VY_ERR_RANGE:
            break
        _lib.check(rc)
        table.append((r.name.decode(), int(r.offset), int(r.bytes), int(r.span)))
    check_table(table, plan_bytes(lib, handle, plan, shape))
    return table


def pattern(lo, hi):
    """The poison bytes of buffer positions [lo, hi)"""
    return np.resize(np.roll(POISON_BYTES, -(lo % 4)), hi - lo)


def holes(table):
    """[(region index, first byte, end)] of every stretch of the bound bytes that no launch may touch: behind each region's
    used bytes up to the next region"""
    return [(i, off + used, off + span) for i, (_, off, used, span) in enumerate(table) if span > used]


def violations(host_bytes, table, band):
    """Every hole or band byte of `host_bytes` (a copy of the whole buffer: band, bound bytes, band) that is no longer
    poison -> [(region name, first stray offset relative to the region's used end, count)].  The front band reports as
    "<front band>" with offsets relative to the first bound byte (negative); the back band — and, where the plan is smaller
    than the buffer, the bytes between its end and the band — against the last region."""
    host_bytes = np.asarray(host_bytes).view(np.uint8).reshape(-1)
    check_table(table, host_bytes.size - 2 * band, exact=False)
    out = []

    def stray(lo, hi):
        """positions of the bytes of [lo, hi) that are not poison — whole words first, bytes only where a word differs"""
        a = min(lo + (-lo % 4), hi)
        b = a + (hi - a) // 4 * 4
        found = [lo + np.nonzero(host_bytes[lo:a] != pattern(lo, a))[0]]
        words = np.nonzero(host_bytes[a:b].view(np.uint32) != POISON)[0]
        if words.size:
            w, k = np.nonzero(host_bytes[a:b].reshape(-1, 4)[words] != POISON_BYTES)
            found.append(a + 4 * words[w] + k)
        found.append(b + np.nonzero(host_bytes[b:hi] != pattern(b, hi))[0])
        return np.concatenate(found)

    def scan(name, lo, hi, origin):
        bad = stray(lo, hi)
        if bad.size:
            out.append((name, int(bad[0] - origin), int(bad.size)))

    scan("<front band>", 0, band, band)
    for i, lo, hi in holes(table):
        scan(table[i][0], band + lo, band + hi, band + table[i][1] + table[i][2])
    name, off, used, span = table[-1]
    scan(name, band + off + span, host_bytes.size, band + off + used)
    return out


def gap_bytes(table):
    return sum(hi - lo for _, lo, hi in holes(table))


# ---- device side (torch)
def _fill(buf, lo, hi):
    """poison bytes [lo, hi) of the uint8 device tensor `buf` (whose storage offset is a multiple of 4), on the current stream"""
    import torch
    head = min(-lo % 4, hi - lo)
    if head:
        buf[lo:lo + head] = torch.from_numpy(pattern(lo, lo + head).copy()).to(buf.device)
    lo += head
    tail = (hi - lo) % 4
    if hi - tail > lo:
        buf[lo:hi - tail].view(torch.int32).fill_(int(np.uint32(POISON).view(np.int32)))
    if tail:
        buf[hi - tail:hi] = torch.from_numpy(pattern(hi - tail, hi).copy()).to(buf.device)


def banded(need, band=BAND, zero=False):
    """(buffer, view): a uint8 device buffer of band + need + band bytes, poison all over, and the view of exactly `need`
    bytes inside it (zero: zero-filled, as the gradient and momentum buffers start).  band and need: multiples of 256."""
    import torch
    assert need % 4 == 0 and band % 256 == 0
    buf = torch.empty(band + need + band, dtype=torch.uint8, device="cuda")
    _fill(buf, 0, buf.numel())
    view = buf[band:band + need]
    if zero:
        view.zero_()
    return buf, view


def poison(ws_view, table):
    """After a bind (which zeroes the plan's bytes, gaps included): every hole of the table back to poison, and what the
    view holds behind the plan's end, on the current stream — the one the net launches on."""
    assert ws_view.storage_offset() % 4 == 0
    for _, lo, hi in holes(table):
        _fill(ws_view, lo, hi)
    end = table[-1][1] + table[-1][3]
    if end < ws_view.numel():
        _fill(ws_view, end, ws_view.numel())
