"""Generates tests/golden/reference_go_names.json: the names tests/test_go_shim.py checks the Go shim and the evaluator overlays against,
read from a checkout of the reference module (v1.3.1), so that those checks run without it.  Names only, no source text:

- ring_exported: the exported identifiers of every non-test file of ring/ (tools/go_surface.py, the input of go/ring/SURFACE.md);
- evaluator_signatures: parameter types and results of the methods on *evaluator in ckks/evaluator.go and bfv/evaluator.go;
- upstream_identifiers_found: which of test_go_shim.UPSTREAM_IDENTIFIERS occur in the non-test sources of ckks/ and bfv/.

    python tests/golden/make_reference_go_names.py LATTIGO_CHECKOUT     # rewrites the JSON next to this file
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_go_shim  # noqa: E402


def _go_surface():
    spec = importlib.util.spec_from_file_location("go_surface", os.path.join(ROOT, "tools", "go_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(reference):
    sigs, found = {}, {}
    for pkg, idents in test_go_shim.UPSTREAM_IDENTIFIERS.items():
        d = os.path.join(reference, pkg)
        sigs[pkg] = test_go_shim.evaluator_signatures(open(os.path.join(d, "evaluator.go")).read())
        src = "\n".join(open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith(".go") and not f.endswith("_test.go"))
        found[pkg] = [i for i in idents if i in src]
    return {"reference": "github.com/ldsec/lattigo v1.3.1", "ring_exported": _go_surface().ring_exported(reference),
            "evaluator_signatures": sigs, "upstream_identifiers_found": found}


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    out = os.path.join(HERE, "reference_go_names.json")
    json.dump(build(sys.argv[1]), open(out, "w"), indent=1, sort_keys=True)
    print("wrote", out, os.path.getsize(out), "bytes")
