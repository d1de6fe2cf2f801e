"""CPU: tests/guarded_planes.py keeps its promises on host tensors, for every dtype and every placement the GPU tests of the core buffers
(tests/test_gpu_core_buffers.py) request: the pointer has exactly the requested alignment, the content comes back bit for bit, a single byte
written in front of or behind the plane is seen, and so is a single changed byte inside it."""
import numpy as np
import pytest

import guarded_planes as gp

PLACEMENTS = sorted(set(gp.ADMITTED.values()) | {p for ps in gp.BELOW.values() for p in ps})
SHAPES = ((1,), (7,), (3, 5), (2, 3, 3), (0, 4))


def _array(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    raw = rng.integers(0, 256, size=n * np.dtype(dtype).itemsize, dtype=np.uint8)  # any bit pattern, NaNs included
    return raw.view(dtype).reshape(shape)


def test_the_tables_name_one_alignment_and_one_step_below():
    for name, (offset, modulus) in gp.ADMITTED.items():
        assert 0 < offset < modulus and modulus % (2 * (offset & -offset)) == 0, name
    assert [gp.ADMITTED[k][0] for k in ("double2", "double", "word")] == [16, 8, 4]
    for name, below in gp.BELOW.items():
        need = gp.ADMITTED[name][0]
        for offset, modulus in below:
            assert modulus == need and offset % need != 0, (name, offset, modulus)  # refused by a check of `need` bytes
        assert need // 2 in [o for o, _ in below]  # the nearest miss is among them


@pytest.mark.parametrize("dtype", gp.DTYPES)
def test_placement_content_and_guards(dtype):
    for offset, modulus in PLACEMENTS:
        for shape in SHAPES:
            a = _array(dtype, shape, offset * 100 + modulus)
            p = gp.Plane(a, offset, modulus)
            assert p.ptr % modulus == offset
            low = offset & -offset
            assert p.ptr % low == 0 and p.ptr % (2 * low) != 0  # that alignment and not the next power of two
            assert p.start >= gp.MIN_GUARD and p.buf.numel() - p.start - a.nbytes >= gp.MIN_GUARD
            assert p.guards_intact() and p.unchanged()
            got = p.get()
            assert got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == a.tobytes()
            a_before = a.copy()
            got.reshape(-1).view(np.uint8)[:] = 0  # get() hands out a copy: neither the plane nor the caller's array follows it
            assert p.unchanged() and a.tobytes() == a_before.tobytes()


def test_default_modulus_is_twice_the_lowest_set_bit():
    for offset in (1, 2, 4, 8, 16, 32, 64):
        p = gp.Plane(np.arange(5, dtype=np.float32), offset)
        assert p.ptr % (2 * offset) == offset and p.align == offset
    with pytest.raises(AssertionError):
        gp.Plane(np.zeros(3), 0)  # offset 0 would be aligned to every power of two up to the allocator's
    with pytest.raises(AssertionError):
        gp.Plane(np.zeros(3), 8, 8)  # 8 modulo 8 is 0
    with pytest.raises(AssertionError):
        gp.Plane(np.zeros(3), 4, 4)


@pytest.mark.parametrize("dtype", gp.DTYPES)
def test_fresh_is_guard_in_every_byte(dtype):
    for offset, modulus in PLACEMENTS:
        f = gp.fresh((3, 4), dtype, offset, modulus)
        assert (f.buf.numpy() == gp.GUARD).all() and f.unchanged()
        got = f.get()
        assert got.shape == (3, 4) and got.dtype == np.dtype(dtype) and (got.reshape(-1).view(np.uint8) == gp.GUARD).all()
        assert got.reshape(-1)[0].tobytes() == gp.guard_value(dtype).tobytes()
    assert gp.guard_value(np.uint8) == 0xCD and gp.guard_value(np.int32) != 0 and gp.guard_value(np.float64) != 0.0 and gp.guard_value(np.float32) != 0.0


@pytest.mark.parametrize("dtype", gp.DTYPES)
def test_a_planted_byte_is_seen(dtype):
    """one byte right in front of the plane, right behind it, at the far ends of both guards; one byte inside the plane"""
    for offset, modulus in PLACEMENTS:
        a = _array(dtype, (3, 5), offset)
        n = a.nbytes
        for where in ("first guard byte", "last byte in front", "first byte behind", "last guard byte"):
            p = gp.Plane(a, offset, modulus)
            i = {"first guard byte": 0, "last byte in front": p.start - 1, "first byte behind": p.start + n, "last guard byte": p.buf.numel() - 1}[where]
            p.buf[i] = gp.GUARD ^ 1
            assert not p.guards_intact() and not p.unchanged(), where
            with pytest.raises(AssertionError):
                p.get()
        for i in (0, n // 2, n - 1):
            p = gp.Plane(a, offset, modulus)
            p.buf[p.start + i] = int(p.buf[p.start + i]) ^ 0x10
            assert p.guards_intact() and not p.unchanged(), i
            assert p.get().tobytes() != a.tobytes()
        f = gp.fresh((2, 3), dtype, offset, modulus)
        f.buf[f.start + 1] = 0
        assert f.guards_intact() and not f.unchanged()
