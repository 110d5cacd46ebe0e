"""Generates tests/golden/reference_keygen_names.json: the names tests/test_go_keygen.py checks the key generator overlays
(go/ckks/keygen_device.go, go/bfv/keygen_device.go) against, read from a checkout of the reference module (v1.3.1), so that those checks run
without it.  Names only, no source text:

- signatures: parameter types and results of the methods on *keyGenerator (and of the function genrotkey) in ckks/keygen.go and bfv/keygen.go;
- fields: the field names of the structs the overlays read (keyGenerator, SwitchingKey, EvaluationKey, RotationKeys, PublicKey, SecretKey);
- upstream_identifiers_found: which of IDENTIFIERS occur in the non-test sources of the package.

    python tests/golden/make_reference_keygen_names.py LATTIGO_CHECKOUT     # rewrites the JSON next to this file
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_go_shim  # noqa: E402

STRUCTS = ["keyGenerator", "SwitchingKey", "EvaluationKey", "RotationKeys", "PublicKey", "SecretKey"]
IDENTIFIERS = {
    "ckks": ["ckksContext", "ringContext", "contextQ", "contextP", "gaussianSampler", "galElRotColLeft", "galElRotColRight", "galElConjugate", "GaloisGen",
             "params.Beta()", "params.LogN", "NewUniformPoly()", "PermuteNTTIndex(", "RotationLeft", "RotationRight", "Conjugate"],
    "bfv": ["bfvContext", "contextQP", "contextQ", "contextP", "gaussianSampler", "galElRotColLeft", "galElRotColRight", "galElRotRow", "params.beta",
            "params.LogN", "NewUniformPoly()", "bfvContext.n", "RotationLeft", "RotationRight", "RotationRow"],
}


def signatures(text):
    """{name: [parameter types, results]} of the methods on *keyGenerator and of the package-level genrotkey"""
    out = {}
    for m in re.finditer(r"func (?:\(\w+ \*keyGenerator\) )?(\w+)\(([^)]*)\)([^{]*)\{", text):
        if "(keygen *keyGenerator)" not in m.group(0) and m.group(1) != "genrotkey":
            continue
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
        out["signatures"][pkg] = signatures(open(os.path.join(d, "keygen.go")).read())
        out["fields"][pkg] = {s: fields(src, s) for s in STRUCTS}
        out["upstream_identifiers_found"][pkg] = [i for i in idents if i in src]
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    target = os.path.join(HERE, "reference_keygen_names.json")
    json.dump(build(sys.argv[1]), open(target, "w"), indent=1, sort_keys=True)
    print("wrote", target, os.path.getsize(target), "bytes")
