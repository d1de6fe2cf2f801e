"""GPU: the mover removal (include/rsdsfm_erase.h) bit for bit against its definition (tests/erase_spec_numpy.py) in both library builds -- the
matte alone at the shapes where its row segments, their halo and its column reach can go wrong, the constructed flags with known answers, the
composite alone at the shapes where its 16 x 64 tile can go wrong and exhaustively over every (a, R, P), the frame call on every case of
tests/erase_cases.py against the golden fixture the CPU suite holds to the definition and against the public calls made one after another with
the own frame rendered separately, the clip call against the frame calls, the workspace across size changes and a growing neighbour count,
every refusal of the header, a seeded random campaign.  Every plane sits at a 4-byte offset that is not 16-byte aligned with guard bytes on
both sides, the outputs are never preset, the inputs are verified unchanged."""
import functools
import os

import numpy as np
import pytest

import denoise_cases as dcases
import erase_cases as cases
import erase_spec_numpy as spec

pytestmark = pytest.mark.gpu

GUARD = 0xCD
FRONT = 20  # bytes of guard in front of a plane: 4-byte aligned, not 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_erase_v1.npz")
PLANES = ("image", "mask", "matte", "moving")


class Plane:
    """a's bytes on the device at a 4-byte offset that is not 16-byte aligned, FRONT guard bytes in front and 28 behind"""

    def __init__(self, torch, dev, a):
        self.host = np.ascontiguousarray(a)
        n = self.host.size
        self.buf = torch.full((FRONT + n + 28,), GUARD, dtype=torch.uint8, device=dev)
        self.buf[FRONT:FRONT + n] = torch.from_numpy(self.host.reshape(-1)).to(dev)
        self.t = self.buf[FRONT:FRONT + n].view(*self.host.shape)
        self.ptr = self.t.data_ptr()
        assert self.ptr % 4 == 0 and self.ptr % 16 != 0

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return (b[:FRONT] == GUARD).all() and (b[FRONT + self.host.size:] == GUARD).all()

    def get(self):
        assert self.guards_intact()
        return self.t.cpu().numpy()

    def unchanged(self):
        return np.array_equal(self.get(), self.host)


def _fresh(torch, dev, shape):
    """an output plane, never preset: every byte GUARD"""
    return Plane(torch, dev, np.full(shape, GUARD, dtype=np.uint8))


def _counters(torch, dev):
    """five int64 at an 8-byte offset that is not 16-byte aligned, a guard word on either side"""
    cnt = torch.full((7,), -1, dtype=torch.int64, device=dev)
    assert cnt[1:].data_ptr() % 16 == 8
    return cnt


def _counts(cnt, with_counts=True):
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and c[6] == -1 and (with_counts or c[1:6] == [-1] * 5)
    return c[1:6]


def _matte(torch, s, flag, o, g, T, und):
    dev = torch.device("cuda", 0)
    d_f, d_a = Plane(torch, dev, flag), _fresh(torch, dev, flag.shape)
    torch.cuda.synchronize()
    s.mover_matte_dev(d_f.ptr, flag.shape[0], flag.shape[1], d_a.ptr, o, g, T, und)
    s.synchronize()
    assert d_f.unchanged()
    return d_a.get()


def _composite(torch, s, ref, rmask, plate, pmask, matte, T, with_counts=True):
    dev = torch.device("cuda", 0)
    rows, cols = rmask.shape
    ins = [Plane(torch, dev, a) for a in (ref, rmask, plate, pmask, matte)]
    d_out, d_mask, cnt = _fresh(torch, dev, ref.shape), _fresh(torch, dev, (rows, cols)), _counters(torch, dev)
    torch.cuda.synchronize()
    s.erase_composite_dev(*[p.ptr for p in ins], 1 if ref.ndim == 2 else 3, rows, cols, d_out.ptr, d_mask.ptr, cnt[1:].data_ptr() if with_counts else None, feather=T)
    s.synchronize()
    assert all(p.unchanged() for p in ins)
    return dict(image=d_out.get(), mask=d_mask.get(), counts=_counts(cnt, with_counts))


def _same(got, want, name="", keys=("image", "mask"), counts=True):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (name, k)
    assert not counts or list(got["counts"]) == list(want["counts"]), (name, got["counts"], want["counts"])


# the definition once per input, shared by both builds and never changed
@functools.lru_cache(maxsize=None)
def _wanted_matte(shape, k, und):
    o, g, T = cases.MATTE_PARAMETERS[k]
    return spec.matte(cases.random_flag(shape, k), o, g, T, und)


@functools.lru_cache(maxsize=None)
def _wanted_constructed():
    return [[spec.matte(F, *p) for p in params] for _, F, params, _ in cases.constructed_flags()]


@functools.lru_cache(maxsize=None)
def _wanted_composite(shape, channels, T):
    return spec.composite(*cases.composite_inputs(shape, channels, T), T)


@functools.lru_cache(maxsize=None)
def _wanted_exhaustive(T):
    return spec.composite(*cases.exhaustive_composite(T), T)


# ---------------------------------------------------------------------------------------------------
# the matte
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_matte_equals_the_definition(rsdsfm, arith):
    """every shape -- one word, odd sizes, both sides of the tile, rows that start on every byte of a dword, one under, exactly one and one over
    the row pass's segment of 1024 and two segments and a rest, frames lower than the column pass's reach at cols % 4 != 0 and == 0 --; no
    cleaning at all, the defaults, the largest reach, and each of open, grow and feather alone; flag bytes from 0 .. 255; with and without the
    undecided pixels; the sizes change again and again on ONE context"""
    import torch

    values = set()
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.MATTE_SHAPES:
            for k, (o, g, T) in enumerate(cases.MATTE_PARAMETERS):
                F = cases.random_flag(shape, k)
                for und in (0, 1):
                    want = _wanted_matte(shape, k, und)
                    assert np.array_equal(_matte(torch, s, F, o, g, T, und), want), (shape, o, g, T, und)
                    values |= set(np.unique(want).tolist())
            assert rsdsfm.mover_matte_launches(*shape) == 3
    assert values == set(range(17))


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_constructed_flags_have_their_known_mattes(rsdsfm, arith):
    """single seeds at the corners and on both sides of the tile and segment borders, all seeds, all undecided, none, and a block in every
    corner that survives open = 3 because nothing outside the frame vetoes"""
    import torch

    wanted = _wanted_constructed()
    with rsdsfm.Solver(0, arith=arith) as s:
        for (name, F, params, want), specs in zip(cases.constructed_flags(), wanted):
            for i, (p, by_spec) in enumerate(zip(params, specs)):
                got = _matte(torch, s, F, *p, 0)
                assert np.array_equal(got, by_spec), (name, p)
                assert i or want is None or np.array_equal(got, want), name
        assert (_matte(torch, s, np.full((18, 2050), 3, dtype=np.uint8), 3, 8, 16, 1) == 16).all()


# ---------------------------------------------------------------------------------------------------
# the composite
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_composite_equals_the_definition(rsdsfm, arith, channels):
    """every shape of the 16 x 64 tile; T 1, 3, 4, 7, 16; masks with values other than 0 / 1, random bytes under unset masks, matte bytes above
    T, groups of four pixels without any matte, full of it and mixed; with and without the counters"""
    import torch

    seen = np.zeros(5, dtype=np.int64)
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.ACC_SHAPES:
            for T in cases.FEATHERS:
                inputs = cases.composite_inputs(shape, channels, T)
                want = _wanted_composite(shape, channels, T)
                _same(_composite(torch, s, *inputs, T), want, (shape, T))
                _same(_composite(torch, s, *inputs, T, with_counts=False), want, (shape, T, "no counters"), counts=False)
                seen += np.array(want["counts"])
        assert rsdsfm.erase_composite_launches() == 1
    assert (seen > 0).all()


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_composite_over_every_matte_byte_and_pair_of_bytes(rsdsfm, arith):
    """one gray frame per T that holds every (a, R, P): the division by T through its reciprocal is exact everywhere"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        for T in cases.FEATHERS:
            want = _wanted_exhaustive(T)
            _same(_composite(torch, s, *cases.exhaustive_composite(T), T), want, T)
            assert want["counts"] == [0, 65536, 65536, (T - 1) * 65536, 0]


def test_the_host_conveniences(rsdsfm):
    F = cases.random_flag((37, 67), 1)
    ref, rmask, plate, pmask, matte = cases.composite_inputs((37, 67), 3, 4)
    with rsdsfm.Solver(0) as s:
        assert np.array_equal(s.mover_matte(F), spec.matte(F)) and np.array_equal(s.mover_matte(F, 1, 0, 7, True), spec.matte(F, 1, 0, 7, 1))
        img, mask, counts = s.erase_composite(ref, rmask, plate, pmask, matte)
        _same(dict(image=img, mask=mask, counts=counts.tolist()), spec.composite(ref, rmask, plate, pmask, matte))


def test_a_seeded_random_campaign(rsdsfm):
    """40 mattes and 20 composites: shapes up to 40 x 1100, every parameter, sparse to dense seeds (tests/test_erase_cpu.py holds the generators
    to their promise)"""
    import torch

    rng = np.random.default_rng(20261)
    with rsdsfm.Solver(0) as s:
        for k in range(40):
            case = cases.random_matte_case(rng)
            got = _matte(torch, s, case["flag"], case["open"], case["grow"], case["feather"], case["include_undecided"])
            assert np.array_equal(got, cases.matte_of(case)), (k, case["flag"].shape, case["open"], case["grow"], case["feather"], case["include_undecided"])
        for k in range(20):
            case = cases.random_composite_case(rng)
            _same(_composite(torch, s, case["ref"], case["rmask"], case["plate"], case["pmask"], case["matte"], case["feather"]), cases.composite_of(case), k)


# ---------------------------------------------------------------------------------------------------
# the refusals of the two primitives
# ---------------------------------------------------------------------------------------------------
def test_matte_and_composite_argument_errors(rsdsfm):
    """every refusal returns RSDSFM_ERR_INVALID and enqueues nothing: the outputs keep their guard bytes; after a refused call the same call
    without the fault goes through"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, T = 16, 64, 4
    ref, rmask, plate, pmask, matte = cases.composite_inputs((rows, cols), 3, T)
    flag = cases.random_flag((rows, cols), 0)
    d = {k: Plane(torch, dev, a) for k, a in dict(ref=ref, rmask=rmask, plate=plate, pmask=pmask, matte=matte, flag=flag).items()}
    out, omask, amatte, cnt = _fresh(torch, dev, ref.shape), _fresh(torch, dev, (rows, cols)), _fresh(torch, dev, (rows, cols)), _counters(torch, dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        def mat(f=d["flag"].ptr, r=rows, c=cols, a=amatte.ptr, o=2, g=2, t=T, u=0):
            return s.mover_matte_dev(f, r, c, a, o, g, t, u)

        def com(R=d["ref"].ptr, mR=d["rmask"].ptr, P=d["plate"].ptr, mP=d["pmask"].ptr, a=d["matte"].ptr, ch=3, r=rows, c=cols, o=out.ptr, k=omask.ptr,
                n=cnt[1:].data_ptr(), t=T):
            return s.erase_composite_dev(R, mR, P, mP, a, ch, r, c, o, k, n, feather=t)

        bad_matte = (dict(f=0), dict(a=0), dict(a=d["flag"].ptr), dict(f=d["flag"].ptr + 1), dict(a=amatte.ptr + 2), dict(r=1), dict(c=1), dict(r=16385), dict(c=16385),
                     dict(o=-1), dict(o=4), dict(g=-1), dict(g=9), dict(t=0), dict(t=17), dict(t=-1), dict(u=2), dict(u=-1))
        bad_com = (dict(R=0), dict(mR=0), dict(P=0), dict(mP=0), dict(a=0), dict(o=0), dict(k=0), dict(R=d["ref"].ptr + 1), dict(mR=d["rmask"].ptr + 2),
                   dict(P=d["plate"].ptr + 3), dict(mP=d["pmask"].ptr + 1), dict(a=d["matte"].ptr + 2), dict(o=out.ptr + 1), dict(k=omask.ptr + 2), dict(n=cnt.data_ptr() + 4),
                   dict(o=d["ref"].ptr), dict(o=d["plate"].ptr), dict(k=d["rmask"].ptr), dict(k=d["pmask"].ptr), dict(o=d["matte"].ptr), dict(k=out.ptr), dict(n=out.ptr),
                   dict(mR=d["ref"].ptr), dict(mP=d["plate"].ptr), dict(a=d["ref"].ptr), dict(a=d["pmask"].ptr), dict(mP=d["ref"].ptr),
                   dict(mR=d["plate"].ptr), dict(ch=2), dict(ch=4), dict(r=1), dict(c=16385), dict(r=16385), dict(c=1), dict(t=0), dict(t=17), dict(t=-1))
        for call, bads in ((mat, bad_matte), (com, bad_com)):
            for bad in bads:
                with pytest.raises(rsdsfm.RsdsfmError):
                    call(**bad)
        s.synchronize()
        for p in (out, omask, amatte):  # nothing was enqueued
            assert (p.get() == GUARD).all()
        assert cnt.cpu().numpy().tolist() == [-1] * 7
        for call, bads in ((mat, bad_matte), (com, bad_com)):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bads[0])
            call()  # the same call without the fault goes through
        s.synchronize()
        want = spec.composite(ref, rmask, plate, pmask, matte, T)
        assert np.array_equal(amatte.get(), spec.matte(flag, 2, 2, T)) and np.array_equal(out.get(), want["image"]) and np.array_equal(omask.get(), want["mask"])
        assert _counts(cnt) == want["counts"]
        before = [p.get().copy() for p in (out, omask, amatte)]
        for call, bads in ((mat, bad_matte), (com, bad_com)):  # a refused call leaves a valid call's outputs as they are
            for bad in bads:
                with pytest.raises(rsdsfm.RsdsfmError):
                    call(**bad)
        s.synchronize()
        assert all(np.array_equal(p.get(), b) for p, b in zip((out, omask, amatte), before)) and _counts(cnt) == want["counts"]
        assert all(p.unchanged() for p in d.values())
        com(P=d["ref"].ptr, mP=d["rmask"].ptr)  # the plate may be the reference: the own frame comes back
        s.synchronize()
        on = rmask != 0
        assert np.array_equal(out.get(), np.where(on[..., None], ref, 0)) and _counts(cnt)[4] == 0


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
def _clip(torch, dev, case):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(frames=[tt(x) for x in case["frames"]], maps=[tt(z.T) for z in case["depths"]], Rs=[tt(np.asarray(R).reshape(-1, 9)) for R in case["Rs"]],
                ts=[tt(t) for t in case["ts"]])


def _frame_kw(case):
    return dict(open=case["open"], grow=case["grow"], feather=case["feather"], include_undecided=case["include_undecided"], threshold=case["threshold"],
                min_votes=case["min_votes"], gain=case["gain_mode"] == 0, min_overlap=case["min_overlap"], window=case["window"], occlusion=case["occlusion"],
                occlusion_tol_q16=case["tol_q16"], mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])


def _outputs(torch, dev, case):
    rows, cols = case["depths"][0].shape
    return [_fresh(torch, dev, shape) for shape in (case["frames"][0].shape, (rows, cols), (rows, cols), (rows, cols))], _counters(torch, dev)


def _collect(planes, cnt, with_matte=True, with_moving=True, with_counts=True):
    out = {k: p.get() for k, p in zip(PLANES, planes)}
    assert with_matte or (out["matte"] == GUARD).all()
    assert with_moving or (out["moving"] == GUARD).all()
    return dict(out, counts=_counts(cnt, with_counts))


def _keys(with_matte=True, with_moving=True):
    return ("image", "mask") + (("matte",) if with_matte else ()) + (("moving",) if with_moving else ())


def _frame(torch, s, case, d=None, q=None, with_matte=True, with_moving=True, with_counts=True):
    """one rsdsfm_erase_frame_dev of frame q of a case (the context's knob set to the case's) into guarded, never preset outputs"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    planes, cnt = _outputs(torch, dev, case)
    torch.cuda.synchronize()
    s.set_occlusion_search(case["search"])
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    s.erase_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, planes[0].ptr, planes[1].ptr, planes[2].ptr if with_matte else None,
                      planes[3].ptr if with_moving else None, cnt[1:].data_ptr() if with_counts else None, **_frame_kw(case))
    s.synchronize()
    s.set_occlusion_search(0)
    for t, a in zip(d["frames"], case["frames"]):
        assert np.array_equal(t.cpu().numpy(), a)
    return _collect(planes, cnt, with_matte, with_moving, with_counts)


def _parts(torch, s, case):
    """the public calls one after another on planes of the test's own: rsdsfm_plate_frame_dev (plate, its mask, the flag), the own frame's window
    render with id 1 onto zeroed planes -- a render of its own, not the plate's --, rsdsfm_mover_matte_dev, rsdsfm_erase_composite_dev"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    d_plate, d_pmask = _fresh(torch, dev, case["frames"][0].shape), _fresh(torch, dev, (rows, cols))
    d_ref, d_rm = Plane(torch, dev, np.zeros_like(case["frames"][0])), Plane(torch, dev, np.zeros((rows, cols), dtype=np.uint8))
    planes, cnt = _outputs(torch, dev, case)
    torch.cuda.synchronize()
    s.plate_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, d_plate.ptr, d_pmask.ptr, None, planes[3].ptr, None,
                      threshold=case["threshold"], min_votes=case["min_votes"], gain=case["gain_mode"] == 0, min_overlap=case["min_overlap"], window=case["window"],
                      occlusion=case["occlusion"], occlusion_tol_q16=case["tol_q16"], mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    s.stabilize_window_frame_dev(d["frames"][src[0]].data_ptr(), ch, d["maps"][src[0]].data_ptr(), d["Rs"][src[0]].data_ptr(), d["ts"][src[0]].data_ptr(), case["K"], rows, cols,
                                 M[0], m[0], 1, case["window"], d_ref.ptr, d_rm.ptr, mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    s.mover_matte_dev(planes[3].ptr, rows, cols, planes[2].ptr, case["open"], case["grow"], case["feather"], case["include_undecided"])
    s.erase_composite_dev(d_ref.ptr, d_rm.ptr, d_plate.ptr, d_pmask.ptr, planes[2].ptr, ch, rows, cols, planes[0].ptr, planes[1].ptr, cnt[1:].data_ptr(), feather=case["feather"])
    s.synchronize()
    assert d_plate.guards_intact() and d_pmask.guards_intact() and d_ref.guards_intact() and d_rm.guards_intact()
    return _collect(planes, cnt)


def _golden(g, name):
    return dict({k: g[name + "/" + k] for k in PLANES}, counts=g[name + "/counts"].tolist())


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_every_case_equals_the_definition_and_the_public_calls(oracle, rsdsfm, arith):
    """image, mask, matte, flag and the five counts of every fixture case -- the plate's clips, each with another set of matte parameters --
    against the golden fixture (the definition's erase_frame) and against the public calls made one after another with the own frame rendered
    separately; the launch count.  The cases change the frame size again and again on ONE context and bring more neighbours than any before:
    the workspace is released and regrown"""
    import torch

    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        every = cases.all_cases(oracle.pose_table)
        for case in every:
            n = case["name"]
            want = _golden(g, n)
            _same(_frame(torch, s, case), want, n, PLANES)
            s.set_occlusion_search(case["search"])
            parts = _parts(torch, s, case)
            s.set_occlusion_search(0)
            _same(parts, want, n + " parts", PLANES)
            nsrc = len(dcases.sources_and_poses(case)[0])
            rows, cols = case["depths"][0].shape
            assert rsdsfm.erase_launches(rows, cols, nsrc) == rsdsfm.plate_launches(rows, cols, nsrc) + rsdsfm.mover_matte_launches(rows, cols) + rsdsfm.erase_composite_launches()
        # fewer neighbours after more at the same size: the larger stack is kept; then back to sizes seen before; a matte alone in between
        by_name = {c["name"]: c for c in every}
        for n in ("five-middle", "five-first", "five-middle", "gained", "2x2", "five-radius-7"):
            _same(_frame(torch, s, by_name[n]), _golden(g, n), n + " again", PLANES)
            F = cases.random_flag((19, 70), 3)
            assert np.array_equal(_matte(torch, s, F, 1, 2, 4, 0), spec.matte(F, 1, 2, 4))
        case = by_name["gained"]
        want = _golden(g, "gained")
        for matte, moving, counts in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            _same(_frame(torch, s, case, with_matte=matte, with_moving=moving, with_counts=counts), want, "optional outputs", _keys(matte, moving), counts)


def test_the_mover_scene_on_the_gpu(rsdsfm):
    """the scenes of tests/test_erase_cpu.py's quality tests through the frame call: the definition's bytes"""
    import torch

    with rsdsfm.Solver(0) as s:
        for hot in (False, True):
            case, prints = cases.mover_scene(hot_pixel=hot)
            for o, g, T in cases.MOVER_PARAMETERS[:2] if hot else cases.MOVER_PARAMETERS:
                c = dict(case, open=o, grow=g, feather=T)
                got = _frame(torch, s, c)
                _same(got, cases.run_spec(c), ("mover", hot, o, g, T), PLANES)
                assert got["counts"][2] >= prints[case["q"]].sum()


def test_frame_argument_errors(oracle, rsdsfm):
    """a refused frame call enqueues nothing: the outputs keep their guard bytes"""
    import torch

    dev = torch.device("cuda", 0)
    case = [c for c in cases.all_cases(oracle.pose_table) if c["name"] == "gained"][0]
    rows, cols = case["depths"][0].shape
    d = _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case)
    planes, cnt = _outputs(torch, dev, case)
    torch.cuda.synchronize()
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    with rsdsfm.Solver(0) as s:
        def call(images=pick("frames"), maps=pick("maps"), M=M, m=m, o=planes[0].ptr, k=planes[1].ptr, a=planes[2].ptr, f=planes[3].ptr, cnt_=cnt[1:].data_ptr(), ch=3, **kw):
            return s.erase_frame_dev(images, ch, maps, pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, o, k, a, f, cnt_, **kw)

        def params(**fields):
            p = rsdsfm._erase_params()
            for name, value in fields.items():
                if name == "reserved":
                    p.reserved[value] = 1
                else:
                    setattr(p, name, value)
            return dict(params=p)

        bad_M = M.copy()
        bad_M[1, 0, 0] = np.nan
        bads = (dict(images=[0] + pick("frames")[1:]), dict(maps=pick("maps")[:2] + [0]), dict(images=[]),
                dict(images=pick("frames") * 6, maps=pick("maps") * 6, M=np.tile(M, (6, 1, 1)), m=np.tile(m, (6, 1))), dict(M=bad_M), dict(o=0), dict(k=0),
                dict(o=planes[1].ptr), dict(a=planes[0].ptr), dict(f=planes[2].ptr), dict(o=planes[0].ptr + 1), dict(k=planes[1].ptr + 2),
                dict(a=planes[2].ptr + 1), dict(f=planes[3].ptr + 2), dict(cnt_=cnt.data_ptr() + 4), dict(o=pick("frames")[2]), dict(k=pick("frames")[0]),
                dict(a=pick("frames")[1]), dict(f=pick("frames")[1]), dict(images=[pick("frames")[0] + 1] + pick("frames")[1:]), dict(ch=2), dict(threshold=256),
                dict(threshold=-1), dict(min_votes=16), dict(min_votes=-1), dict(min_overlap=-1), dict(occlusion=2), dict(occlusion=True, occlusion_tol_q16=65537),
                dict(window=(0, 0, rows + 1, cols)), dict(window=(1, 1, 0, 4)), dict(iterations=17), dict(open=4), dict(grow=9), dict(feather=17), dict(feather=-1),
                dict(include_undecided=2), params(open=-2), params(grow=-2), params(struct_bytes=56), params(reserved=0), params(reserved=4), params(radius=8),
                params(include_undecided=-1))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        for p in planes:
            assert (p.get() == GUARD).all()
        assert cnt.cpu().numpy().tolist() == [-1] * 7
        kw = {k: v for k, v in _frame_kw(case).items() if k not in ("window", "occlusion", "occlusion_tol_q16", "mode", "q5_mode", "iterations")}
        call(**kw)
        s.synchronize()
        want = cases.run_spec(case)
        _same(_collect(planes, cnt), want, "after the refusals", PLANES)
        # the struct's 0 is the default and its -1 is none
        call(**params(open=0, grow=0, feather=0, threshold=case["threshold"], min_votes=case["min_votes"]))
        s.synchronize()
        _same(_collect(planes, cnt), cases.run_spec(dict(case, open=2, grow=2, feather=4, include_undecided=0)), "struct defaults", PLANES)
        call(**params(open=-1, grow=-1, feather=1, struct_bytes=0, threshold=case["threshold"], min_votes=case["min_votes"]))
        s.synchronize()
        got = _collect(planes, cnt)
        _same(got, cases.run_spec(dict(case, open=0, grow=0, feather=1, include_undecided=0)), "struct none", PLANES)
        assert np.array_equal(got["matte"], (got["moving"] == 2).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------
# the clip call
# ---------------------------------------------------------------------------------------------------
def _video(torch, s, case, want_counts=True, with_optional=True):
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    ns = len(case["depths"])
    d = _clip(torch, dev, case)
    outs = [_outputs(torch, dev, case) for _ in range(ns)]
    torch.cuda.synchronize()
    ptrs = lambda a: [x.data_ptr() for x in a]
    s.set_occlusion_search(case["search"])
    r = s.erase_video_dev(ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"], case["c_path"],
                          case["scales"], [p[0].ptr for p, _ in outs], [p[1].ptr for p, _ in outs], [p[2].ptr for p, _ in outs] if with_optional else None,
                          [p[3].ptr for p, _ in outs] if with_optional else None, want_counts=want_counts, radius=case["radius"], **_frame_kw(case))
    s.synchronize()
    s.set_occlusion_search(0)
    got = []
    for q, (planes, cnt) in enumerate(outs):
        one = _collect(planes, cnt, with_optional, with_optional, False)
        one["counts"] = r["counts"][q].tolist() if want_counts else None
        got.append(one)
    return got, d


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(oracle, rsdsfm, arith):
    """three sources (radius 1), five (radius 2: the first and last frames with one-sided neighbours) and one source alone: every frame of the
    clip call is the frame call's, which is the definition's; without the counters, the mattes and the flag planes the call only enqueues; a
    refused clip call enqueues nothing"""
    import torch

    every = {c["name"]: c for c in cases.all_cases(oracle.pose_table)}
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in (every["gained"], every["five-middle"], every["one-source-undecided"], dict(every["fold-search"], radius=2)):
            got, d = _video(torch, s, case)
            for q in range(len(case["depths"])):
                want = cases.run_spec(case, q)
                _same(got[q], want, (case["name"], q), PLANES)
                _same(_frame(torch, s, case, d, q), want, (case["name"], q, "frame"), PLANES)
        case = every["five-middle"]
        got, _ = _video(torch, s, case, want_counts=False, with_optional=False)
        for q in range(5):
            _same(got[q], cases.run_spec(case, q), q, counts=False)
        dev = torch.device("cuda", 0)
        rows, cols = case["depths"][0].shape
        d = _clip(torch, dev, case)
        outs = [_outputs(torch, dev, case) for _ in range(5)]
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        bad_scales = case["scales"].copy()
        bad_scales[4] = 0.0

        def call(scales=case["scales"], o=None, a=None, **kw):
            return s.erase_video_dev(ptrs(d["frames"]), rows, cols, 1, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                     case["c_path"], scales, o or [p[0].ptr for p, _ in outs], [p[1].ptr for p, _ in outs], a, None, **kw)

        for bad in (dict(scales=bad_scales), dict(radius=8), dict(radius=-1), dict(threshold=300), dict(open=4), dict(grow=9), dict(feather=17),
                    dict(o=[outs[0][0][0].ptr] * 4 + [0]), dict(o=[outs[0][0][0].ptr] * 4 + [d["frames"][1].data_ptr()]), dict(a=[outs[0][0][2].ptr] * 4 + [0])):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        for planes, cnt in outs:
            assert all((p.get() == GUARD).all() for p in planes) and cnt.cpu().numpy().tolist() == [-1] * 7


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
def test_evaluate_real_sequence_with_erase(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, erase=True, K or (K, open, grow, feather)) on a small synthetic clip with a mover adds exactly
    erased, erase_matte and erase_counts and the files erased_<p>.png, matte_<p>.png and erase.csv, and the arrays are Solver.erase_video_dev's on
    the clip's own outputs; without the keyword every key and file is what it was; without stabilize=True it raises ValueError"""
    import torch

    from test_gpu_stabilize_search import TRIALS, plain_clip

    _, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    v, w, k = rsdsfm.synth.default_motion()
    sc = 4.0 / np.abs(rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)[0]).max()
    mover = (5, 16, 4, 6, 5, 1)  # plain_clip's render with something that moves through the static scene
    frames = list(rsdsfm.synth.render_sequence(3, rows, cols, K, v * sc, w * sc, k, gamma, seed=21, speeds=(1.0, 1.3), mover=mover)[0])
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0) as s:
        with pytest.raises(ValueError):
            ev(s, frames, erase=True, **dict(kw, stabilize=False))
        out = ev(s, frames, erase=(1, 0, 1, 3), out_dir=str(tmp_path / "with"), **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "without"), **kw)
        default = ev(s, frames, erase=True, **kw)
        ps, o = out["path_smoothed"], out["pairs"]
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_f, d_z = [tt(frames[q]) for q in range(n)], [tt(np.asarray(o[q]["depth_map"]).T) for q in range(n)]
        d_R, d_t = [tt(np.asarray(o[q]["R"]).reshape(-1, 9)) for q in range(n)], [tt(o[q]["t"]) for q in range(n)]
        case = dict(frames=frames, depths=[np.empty((rows, cols))])
        outs = [_outputs(torch, dev, case) for _ in range(n)]
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        r = s.erase_video_dev(ptrs(d_f), rows, cols, 3, K, ptrs(d_z), ptrs(d_R), ptrs(d_t), out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], [p[0].ptr for p, _ in outs],
                              [p[1].ptr for p, _ in outs], [p[2].ptr for p, _ in outs], None, radius=1, open=0, grow=1, feather=3)
        s.synchronize()
        direct = [_collect(p, c, True, False, False) for p, c in outs]
    new = {"erased", "erase_matte", "erase_counts"}
    assert set(out) == set(plain) | new == set(default)
    assert len(out["erased"]) == len(out["erase_matte"]) == n and out["erase_counts"].shape == (n, 5)
    for p in range(n):
        assert np.array_equal(out["erased"][p], direct[p]["image"]) and np.array_equal(out["erase_matte"][p], direct[p]["matte"])
        assert out["erase_counts"][p].tolist() == r["counts"][p].tolist() and out["erase_counts"][p].sum() == rows * cols
        assert out["erased"][p].shape == frames[0].shape and out["erase_matte"][p].max() <= 3
    for key in plain:
        if key not in ("pairs", "path_smoothed", "links"):
            assert np.asarray(out[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    with_files, without_files = set(os.listdir(str(tmp_path / "with"))), set(os.listdir(str(tmp_path / "without")))
    assert with_files == without_files | {"erased_%d.png" % p for p in range(n)} | {"matte_%d.png" % p for p in range(n)} | {"erase.csv"}
    lines = open(str(tmp_path / "with" / "erase.csv")).read().split()
    assert lines[0] == "pair,unset,kept,replaced,feathered,unresolved" and len(lines) == 1 + n
    assert lines[1].split(",") == ["0"] + [str(int(x)) for x in out["erase_counts"][0]]
