"""Device (or host) planes for tests of the C ABI's device entry points: an array of any dtype placed at a chosen byte offset modulo a
power of two inside a larger byte buffer that is filled with GUARD, so that

  * the pointer a kernel gets has EXACTLY the alignment the header admits (offset 16 modulo 32 is 16-byte aligned and not 32-byte aligned;
    offset 4 modulo 8 is 4-byte aligned and not 8; offsets 1, 2, 3 modulo 4 for planes that may sit anywhere), or one step below it for a
    refusal test -- a torch allocation alone is 256-byte aligned and hides every alignment assumption;
  * a store in front of or behind the plane lands in guard bytes and is seen (guards_intact);
  * an output is never preset: fresh() is GUARD in every byte, so an element a kernel leaves unwritten is seen;
  * an input is verified unchanged (unchanged()).

The plane is kept as BYTES on the device (a typed torch view of a misaligned address does not exist); get() copies them back and
reinterprets them on the host.  A device plane is complete when its constructor returns (it synchronises the device: torch fills it on its own
stream, the library works on another), so a pointer may go straight into a call on any stream.  A plain module, no fixture: `from guarded_planes import Plane, fresh`."""
import numpy as np

GUARD = 0xCD
MIN_GUARD = 64  # bytes of guard on either side, at least

# offset -> modulus of every placement the GPU tests of the core buffers request (tests/test_gpu_core_buffers.py); the CPU test of this
# module (tests/test_guarded_planes_cpu.py) holds the helper to its promises on exactly these
ADMITTED = {"double2": (16, 32), "double": (8, 16), "word": (4, 8), "byte1": (1, 4), "byte2": (2, 4), "byte3": (3, 4)}
BELOW = {"double2": ((8, 16), (4, 16)), "double": ((4, 8),), "word": ((1, 4), (2, 4))}  # one step below a need of 16 / 8 / 4 bytes
DTYPES = (np.uint8, np.int32, np.float32, np.int64, np.float64)


def _lowbit(x):
    return x & -x


class Plane:
    """`a`'s bytes at an address that is `offset` modulo `modulus` (default: twice the lowest set bit of `offset`, which makes the pointer
    aligned to that bit and to no higher power of two), at least MIN_GUARD guard bytes in front and behind.  device: a torch device or "cpu"."""

    def __init__(self, a, offset, modulus=None, device="cpu"):
        import torch

        a = np.asarray(a)
        self.host = np.ascontiguousarray(a).copy()
        self.dtype, self.shape = self.host.dtype, self.host.shape
        self.nbytes = self.host.nbytes
        modulus = 2 * _lowbit(offset) if modulus is None else modulus
        assert offset > 0 and modulus & (modulus - 1) == 0 and 0 < offset < modulus and modulus % (2 * _lowbit(offset)) == 0, (offset, modulus)
        self.buf = torch.full((MIN_GUARD + modulus + self.nbytes + MIN_GUARD,), GUARD, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.start = MIN_GUARD + (offset - base - MIN_GUARD) % modulus
        if self.nbytes:
            self.buf[self.start:self.start + self.nbytes] = torch.from_numpy(self.host.reshape(-1).view(np.uint8)).to(device)
        self.ptr = base + self.start
        self.align = _lowbit(offset)
        # exactly the requested alignment: the address modulo, and therefore NOT the next power of two
        assert self.ptr % modulus == offset and self.ptr % self.align == 0 and self.ptr % (2 * self.align) != 0, (self.ptr, offset, modulus)
        assert self.start >= MIN_GUARD and self.buf.numel() - self.start - self.nbytes >= MIN_GUARD
        if self.buf.is_cuda:
            # the guard fill and the copy of the content run on torch's stream, the library on its context's own non-blocking one: nothing
            # else orders the two, so the plane is complete before anybody gets its pointer
            torch.cuda.synchronize(self.buf.device)

    def _bytes(self):
        return self.buf.cpu().numpy()

    def guards_intact(self):
        b = self._bytes()
        return bool((b[:self.start] == GUARD).all() and (b[self.start + self.nbytes:] == GUARD).all())

    def get(self):
        """the plane's current content as a host array of the plane's dtype and shape; fails if a guard byte changed"""
        b = self._bytes()
        assert (b[:self.start] == GUARD).all() and (b[self.start + self.nbytes:] == GUARD).all(), "guard bytes around the plane were overwritten"
        return b[self.start:self.start + self.nbytes].copy().view(self.dtype).reshape(self.shape)

    def unchanged(self):
        """guards intact and every byte of the plane as it was placed (for an input; for a fresh() output: nothing was written)"""
        return self.guards_intact() and bool(np.array_equal(self.get().reshape(-1).view(np.uint8), self.host.reshape(-1).view(np.uint8)))


def fresh(shape, dtype, offset, modulus=None, device="cpu"):
    """an output plane that is never preset: every byte is GUARD"""
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return Plane(np.full(n, GUARD, dtype=np.uint8).view(dtype).reshape(shape), offset, modulus, device)


def guard_value(dtype):
    """what an element of a fresh() plane reads as"""
    return np.full(np.dtype(dtype).itemsize, GUARD, dtype=np.uint8).view(dtype)[0]
