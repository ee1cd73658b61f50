"""Guarded outputs, exact-size workspaces and the two comparisons of the direct C-API tests (tests/test_gpu_bwd_operators.py,
tests/test_gpu_fit_kernels.py): outputs live between sentinel margins and are pre-filled with NaN; workspaces have exactly the
size their *_bytes function states, plus a sentinel page."""
import numpy as np
import torch

SENTINEL, PAGE, PAGE_BYTE = 7.0, 4096, 0xA5
WORST = {}      # what -> worst measured error of this session (printed by every test that raises it)


class Guarded:
    """n elements of `dtype` on the device, pre-filled with NaN, between two margins that hold a sentinel"""

    def __init__(self, n, dev, dtype=torch.float32, margin=256, fill=float("nan")):
        self.n, self.m = n, margin
        self.buf = torch.full((n + 2 * margin,), SENTINEL, dtype=dtype, device=dev)
        self.buf[margin:margin + n] = fill
        self.ptr = self.buf.data_ptr() + margin * self.buf.element_size()

    def read(self, what):
        """the payload as float64 numpy; the margins must be untouched"""
        b = self.buf.double().cpu().numpy()
        assert (b[:self.m] == SENTINEL).all() and (b[self.m + self.n:] == SENTINEL).all(), "%s: wrote outside its output" % what
        return b[self.m:self.m + self.n]


class Workspace:
    """`nbytes` of garbage (quiet NaNs, or zeros) followed by a sentinel page"""

    def __init__(self, nbytes, dev, zero=False):
        assert nbytes > 0 and nbytes % 4 == 0, nbytes
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + PAGE,), PAGE_BYTE, dtype=torch.uint8, device=dev)
        if zero:
            self.buf[:nbytes] = 0
        else:
            self.buf[:nbytes].view(torch.float32).fill_(float("nan"))
        self.ptr = self.buf.data_ptr()

    def check(self, what):
        assert (self.buf[self.nbytes:] == PAGE_BYTE).all().item(), "%s: wrote behind its workspace" % what


def _bits(a):
    return (np.asarray(a, dtype=np.float32) + np.float32(0.0)).view(np.uint32)


def _close(got, ref, what, bmax, bl2=None):
    assert np.isfinite(got).all(), "%s: %d entries not written or not finite" % (what, int((~np.isfinite(got)).sum()))
    top = np.abs(ref).max()
    assert top > 0, what
    emax = float(np.abs(got - ref).max() / top)
    el2 = float(np.linalg.norm((got - ref).ravel()) / np.linalg.norm(ref.ravel()))
    tag = what.split(" ")[0] + (" bf16" if bl2 else "")
    if emax > WORST.get(tag, (-1.0,))[0]:
        WORST[tag] = (emax, el2, what)
        print("  worst so far %-22s max %.2e (bound %.0e) L2 %.2e   at %s" % (tag, emax, bmax, el2, what))
    assert emax <= bmax, "%s: max error %.3e of the largest entry, bound %.1e, at %s" % (
        what, emax, bmax, np.unravel_index(np.abs(got - ref).argmax(), ref.shape))
    if bl2 is not None:
        assert el2 <= bl2, "%s: relative L2 error %.3e, bound %.1e" % (what, el2, bl2)


def _exact(got, ref, what):
    assert np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() < 2 ** 24, what
    ne = _bits(got) != _bits(ref)
    assert not ne.any(), "%s: %d of %d entries differ from the exact result, first at %s: %r instead of %r" % (
        what, int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]), float(got[tuple(np.argwhere(ne)[0])]), float(ref[tuple(np.argwhere(ne)[0])]))
