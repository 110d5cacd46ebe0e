"""Generates tests/golden/reference_collective_names.json: the names tests/test_go_collective.py checks the collective key switching overlays
(go/dckks/keyswitching_device.go, go/dckks/public_keyswitching_device.go, go/dbfv/keyswitching_device.go, go/dbfv/public_keyswitching_device.go)
against, read from a checkout of the reference module (v1.3.1), so that those checks run without it.  Names and arities only, no source text:

- signatures: parameter types and results of the methods on *CKSProtocol and *PCKSProtocol in keyswitching.go and public_keyswitching.go of
  dckks and dbfv;
- fields: the field names of the structs the overlays read (CKSProtocol, PCKSProtocol and the package's context struct);
- upstream_identifiers_found: which of IDENTIFIERS occur in the non-test sources of the package.

    python tests/golden/make_reference_collective_names.py LATTIGO_CHECKOUT     # rewrites the JSON next to this file
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_go_shim  # noqa: E402

FILES = {"CKSProtocol": "keyswitching.go", "PCKSProtocol": "public_keyswitching.go"}
CONTEXT = {"dckks": "dckksContext", "dbfv": "dbfvContext"}
IDENTIFIERS = {
    "dckks": ["dckksContext", "contextQ", "contextP", "contextQP", "gaussianSampler", "gaussianSamplerSmudge", "ct.Level()", "ct.Value()", "ct.Scale()",
              "ctOut.SetScale(", "pk.Get()", "CKSShare", "PCKSShare", "ModDownSplitedNTTPQ(", "ModDownNTTPQ("],
    "dbfv": ["dbfvContext", "contextQ", "contextP", "contextQP", "gaussianSampler", "gaussianSamplerSmudge", "ct.Value()", "pk.Get()", "CKSShare", "PCKSShare",
             "ModDownSplitedPQ(", "ModDownPQ(", "shareOut.Poly"],
}


def signatures(text, receiver):
    """{name: [parameter types, results]} of the methods on *receiver"""
    out = {}
    for m in re.finditer(r"func \(\w+ \*%s\) (\w+)\(([^)]*)\)([^{]*)\{" % receiver, text):
        params = re.sub(r"\s+", " ", m.group(2)).strip()
        types = [re.sub(r"^\w+ ", "", g.strip()) if " " in g.strip() else None for g in test_go_shim._split_args(params)] if params else []
        for i in range(len(types) - 2, -1, -1):       # names without a type take the type of the next typed parameter
            if types[i] is None:
                types[i] = types[i + 1]
        out[m.group(1)] = [types, re.sub(r"\s+", " ", m.group(3)).strip()]
    return out


def fields(src, struct):
    m = re.search(r"type %s struct \{(.*?)\n\}" % struct, src, flags=re.S)
    names = []
    for line in (m.group(1).split("\n") if m else []):
        line = re.sub(r"//.*", "", line).strip()
        if line:
            names += [n.strip() for n in line.split()[0].split(",")] if len(line.split()) > 1 else [line]
    return names


def build(reference):
    out = {"reference": "github.com/ldsec/lattigo v1.3.1", "signatures": {}, "fields": {}, "upstream_identifiers_found": {}}
    for pkg, idents in IDENTIFIERS.items():
        d = os.path.join(reference, pkg)
        src = "\n".join(open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith(".go") and not f.endswith("_test.go"))
        out["signatures"][pkg] = {r: signatures(open(os.path.join(d, f)).read(), r) for r, f in FILES.items()}
        out["fields"][pkg] = {r: fields(open(os.path.join(d, f)).read(), r) for r, f in FILES.items()}
        out["fields"][pkg][CONTEXT[pkg]] = fields(src, CONTEXT[pkg])
        out["upstream_identifiers_found"][pkg] = [i for i in idents if i in src]
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    target = os.path.join(HERE, "reference_collective_names.json")
    json.dump(build(sys.argv[1]), open(target, "w"), indent=1, sort_keys=True)
    print("wrote", target, os.path.getsize(target), "bytes")
