"""Writes tests/golden/binding_calls_v1.json.gz and tests/golden/binding_surface_v1.json.gz: what every call of tests/binding_cases.py hands to the
library and returns, recorded on the stand-in library of tests/binding_recorder.py, and the surface of the binding (names, signatures, structures,
constants); tests/test_binding_marshalling_cpu.py recomputes both.  Needs neither a built library nor a GPU, and writes the same bytes on every
run.  Run from the repository root, on the commit whose binding is the reference:
    python tests/golden/make_golden_binding.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import binding_cases as cases  # noqa: E402
import binding_recorder as rec  # noqa: E402


def main():
    import rsdsfm

    missing = [n for n in rec.dev_methods(rsdsfm) if n not in rec.covered(cases.CASES) and n not in cases.UNCOVERED]
    assert not missing, "no case for %s" % missing
    for name, obj in (("binding_calls_v1.json.gz", rec.build_calls(rsdsfm, cases.CASES, cases.UNCOVERED)),
                      ("binding_surface_v1.json.gz", rec.build_surface(rsdsfm, cases.PRIVATE_SURFACE, ROOT))):
        path = os.path.join(HERE, name)
        rec.write_gz(path, obj)
        print(path, os.path.getsize(path), "bytes,", len(rec.dumps(obj)), "as JSON")
    print(len(cases.CASES), "cases,", len(rec.dev_methods(rsdsfm)), "*_dev methods,", len(cases.UNCOVERED), "uncovered")


if __name__ == "__main__":
    main()
