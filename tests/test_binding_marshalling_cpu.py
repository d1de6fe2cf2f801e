"""CPU: the Python binding hands the library what it handed it when the goldens were written (tests/golden/make_golden_binding.py).

The library is called without argtypes, so a wrapper that builds one argument differently -- a pointer not wrapped, a count as a double, two
arrays swapped, a list cut at another length -- would first show on the GPU, as a fault.  Here every call of tests/binding_cases.py runs on a
stand-in library that records its arguments in a canonical form (tests/binding_recorder.py), and the records, the wrappers' return values, their
refusals' texts and the module's surface are compared with the goldens.  No built library, no GPU.  Not covered: the host conveniences
(Solver.denoise_spatial, .stabilize_filled, ...), which stage their arrays through torch on a device.
"""
import os
import re

import pytest

import binding_cases as cases
import binding_recorder as rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def golden_calls():
    return rec.read_gz(os.path.join(GOLDEN, "binding_calls_v1.json.gz"))


@pytest.fixture(scope="module")
def golden_surface():
    return rec.read_gz(os.path.join(GOLDEN, "binding_surface_v1.json.gz"))


def test_the_table_and_the_golden_list_the_same_cases(golden_calls):
    names = [name for name, _ in cases.CASES]
    assert len(set(names)) == len(names)
    assert sorted(names) == sorted(golden_calls["cases"])


@pytest.mark.parametrize("name,fn", cases.CASES, ids=[name for name, _ in cases.CASES])
def test_case_hands_the_library_the_golden_arguments(rsdsfm, golden_calls, name, fn):
    """the calls in order with every argument's type and value, then the wrapper's return value (keys, dtypes, shapes, contents) or its
    refusal's type and text"""
    want = golden_calls["cases"][name]
    got = rec.loads(rec.dumps(rec.run_case(rsdsfm, fn)))
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert len(g[1]) == len(w[1]), g[0]
        for i, (ga, wa) in enumerate(zip(g[1], w[1])):
            assert ga == wa, "%s argument %d" % (g[0], i)
    assert got.get("raises") == want.get("raises")
    assert got.get("returns") == want.get("returns")


def test_every_dev_method_has_a_case(rsdsfm, golden_calls):
    """a *_dev method of Solver is in the table, or in UNCOVERED with the source it had when the goldens were written: a later stage cannot
    arrive without a case"""
    have = rec.covered(cases.CASES)
    for name in rec.dev_methods(rsdsfm):
        if name in have:
            continue
        assert name in cases.UNCOVERED, "Solver.%s has no case in tests/binding_cases.py" % name
        assert rec.source_sha(vars(rsdsfm.Solver)[name]) == golden_calls["uncovered"].get(name), "Solver.%s changed and has no case" % name
    assert sorted(cases.UNCOVERED) == sorted(golden_calls["uncovered"])


def test_the_surface_holds(rsdsfm, golden_surface):
    """every public name of the module and every private one the tests and tools reach: kind, signature, structure fields and size, constant
    value; every attribute of Solver: signature and docstring"""
    got = rec.loads(rec.dumps(rec.build_surface(rsdsfm, cases.PRIVATE_SURFACE, ROOT)))
    for part in ("module", "solver"):
        assert sorted(got[part]) == sorted(golden_surface[part]), part
        for name in got[part]:
            assert got[part][name] == golden_surface[part][name], "%s %s" % (part, name)


def test_private_names_reached_from_outside_are_in_the_surface():
    """PRIVATE_SURFACE holds every private name the tests, the tools, bench.py and the package's other modules take from the module, by attribute
    or by a relative import"""
    found = set()
    pkg_dir = os.path.join(ROOT, "rs-aware-differential-sfm_amd")
    files = [os.path.join(ROOT, "bench.py")] + [os.path.join(pkg_dir, f) for f in ("evaluate.py", "pipeline.py", "dist.py")]
    for d in ("tests", "tools"):
        files += [os.path.join(base, f) for base, _, fs in os.walk(os.path.join(ROOT, d)) for f in fs if f.endswith(".py")]
    for path in files:
        txt = open(path, errors="replace").read()
        found.update(re.findall(r"\b(?:rsdsfm|pkg)\.(_[a-z][a-zA-Z0-9_]*)", txt))
        for line in re.findall(r"from \. import ([^\n]+)", txt):
            found.update(n.strip() for n in line.split("#")[0].split(",") if n.strip().startswith("_"))
    assert found <= set(cases.PRIVATE_SURFACE), sorted(found - set(cases.PRIVATE_SURFACE))
