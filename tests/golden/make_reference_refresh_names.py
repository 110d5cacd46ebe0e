"""Generates tests/golden/reference_refresh_names.json: the names tests/test_go_refresh.py checks the Refresh overlays
(go/dckks/public_refresh_device.go, go/dbfv/public_refresh_device.go) against, read from a checkout of the reference module (v1.3.1), so
that those checks run without it.  Names and arities only, no source text, in the layout of make_reference_collective_names.py:

- signatures: parameter types and results of the methods on *RefreshProtocol in public_refresh.go of dckks and dbfv;
- fields: the field names of RefreshProtocol and of the package's context struct;
- upstream_identifiers_found: which of IDENTIFIERS occur in the non-test sources of the package.

    python tests/golden/make_reference_refresh_names.py LATTIGO_CHECKOUT     # rewrites the JSON next to this file
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_collective_names import CONTEXT, fields, signatures  # noqa: E402

IDENTIFIERS = {
    "dckks": ["dckksContext", "contextQ", "maskBigint", "gaussianSampler", "ciphertext.Level()", "ciphertext.Value()", "crs.CopyNew()",
              "RefreshShareDecrypt", "RefreshShareRecrypt", "SetCoefficientsBigintLvl(", "PolyToBigint("],
    "dbfv": ["dbfvContext", "contextQ", "contextP", "contextT", "gaussianSampler", "ciphertext.Value()", "ciphertextOut.Value()", "RefreshShare",
             "RefreshShareDecrypt", "RefreshShareRecrypt", "ModDownSplitedPQ(", "ModDownPQ(", "params.T"],
}


def build(reference):
    out = {"reference": "github.com/ldsec/lattigo v1.3.1", "signatures": {}, "fields": {}, "upstream_identifiers_found": {}}
    for pkg, idents in IDENTIFIERS.items():
        d = os.path.join(reference, pkg)
        src = "\n".join(open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith(".go") and not f.endswith("_test.go"))
        text = open(os.path.join(d, "public_refresh.go")).read()
        out["signatures"][pkg] = {"RefreshProtocol": signatures(text, "RefreshProtocol")}
        out["fields"][pkg] = {"RefreshProtocol": fields(text, "RefreshProtocol"), CONTEXT[pkg]: fields(src, CONTEXT[pkg])}
        out["upstream_identifiers_found"][pkg] = [i for i in idents if i in src]
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    target = os.path.join(HERE, "reference_refresh_names.json")
    json.dump(build(sys.argv[1]), open(target, "w"), indent=1, sort_keys=True)
    print("wrote", target, os.path.getsize(target), "bytes")
