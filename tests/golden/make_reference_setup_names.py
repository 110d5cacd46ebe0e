"""Generates tests/golden/reference_setup_names.json: the names tests/test_go_setup.py checks the collective key setup overlays
(publickey_gen_device.go, relinkey_gen_device.go, relinkey_gen_naive_device.go, rotkey_gen_device.go of go/dbfv and go/dckks) against, read
from a checkout of the reference module (v1.3.1), so that those checks run without it.  Names and arities only, no source text, in the
layout of make_reference_collective_names.py:

- signatures: parameter types and results of the methods on *CKGProtocol, *RKGProtocol, *RKGProtocolNaive and *RTGProtocol in
  publickey_gen.go, relinkey_gen.go, relinkey_gen_naive.go and rotkey_gen.go of dbfv and dckks;
- fields: the field names of those four structs and of the package's context struct;
- share_types: what each share type of those files is declared as -- a slice of polys, a slice of pairs, a poly, or a struct.

    python tests/golden/make_reference_setup_names.py LATTIGO_CHECKOUT     # rewrites the JSON next to this file
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_collective_names import CONTEXT, fields, signatures  # noqa: E402

FILES = {"CKGProtocol": "publickey_gen.go", "RKGProtocol": "relinkey_gen.go", "RKGProtocolNaive": "relinkey_gen_naive.go", "RTGProtocol": "rotkey_gen.go"}
KINDS = r"\[\]\*ring\.Poly|\[\]\[2\]\*ring\.Poly|\*ring\.Poly|struct \{"


def build(reference):
    out = {"reference": "github.com/ldsec/lattigo v1.3.1", "signatures": {}, "fields": {}, "share_types": {}}
    for pkg in ("dbfv", "dckks"):
        d = os.path.join(reference, pkg)
        src = "\n".join(open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith(".go") and not f.endswith("_test.go"))
        texts = {r: open(os.path.join(d, f)).read() for r, f in FILES.items()}
        out["signatures"][pkg] = {r: signatures(t, r) for r, t in texts.items()}
        out["fields"][pkg] = {r: fields(t, r) for r, t in texts.items()}
        out["fields"][pkg][CONTEXT[pkg]] = fields(src, CONTEXT[pkg])
        out["share_types"][pkg] = {}
        for r, t in texts.items():
            for m in re.finditer(r"^type (\w+) (%s)" % KINDS, t, flags=re.M):
                if m.group(1) != r:
                    out["share_types"][pkg][m.group(1)] = m.group(2).rstrip(" {")
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    target = os.path.join(HERE, "reference_setup_names.json")
    json.dump(build(sys.argv[1]), open(target, "w"), indent=1, sort_keys=True)
    print("wrote", target, os.path.getsize(target), "bytes")
