"""The BFV encryptor's Go side cannot be compiled here (no Go toolchain in the image): go/ring/bfv_encryptor.go (the cgo types BfvEncryptor /
BfvDecryptor and the compact samplers) and go/bfv/encryptor_device.go, go/bfv/decryptor_device.go (replacement bodies for pkEncryptor.encrypt,
skEncryptor.encrypt and decryptor.Decrypt) are checked statically, in the manner of test_go_bfv_encoder.py -- every C symbol called is
declared in include/lattigo_ring.h with the same number of arguments and every lr_bfv_encrypt* / lr_bfv_decrypt* symbol of the header is
reached, delimiters balance, the go 1.13 language level holds, the overlays call only what the shim has, with its arity, and their methods
keep the upstream signatures (tests/golden/reference_bfv_encryptor_names.json)."""
import json
import os
import re

from conftest import ROOT
from test_go_bfv_encoder import _call_args
from test_go_shim import _header_arity, _split_args, _strip

SHIM = os.path.join(ROOT, "go", "ring", "bfv_encryptor.go")
OVERLAYS = {"encryptor": os.path.join(ROOT, "go", "bfv", "encryptor_device.go"), "decryptor": os.path.join(ROOT, "go", "bfv", "decryptor_device.go")}
NAMES = os.path.join(ROOT, "tests", "golden", "reference_bfv_encryptor_names.json")


def _params(decl):
    """number of parameters of a Go parameter list ("a, b *Poly" declares two)"""
    n = pending = 0
    for g in [g for g in _split_args(decl) if g.strip()]:
        pending += 1
        if len(g.strip().split()) >= 2:
            n += pending
            pending = 0
    return n + pending


def _methods(text, receiver):
    return {m.group(1): _params(m.group(2)) for m in re.finditer(r"func \(\w+ \*%s\) (\w+)\(([^)]*)\)" % receiver, text)}


def test_delimiters_balance_and_packages():
    for path, package in [(SHIM, "ring")] + [(p, "bfv") for p in OVERLAYS.values()]:
        t = _strip(open(path).read())
        for a, b in ("{}", "()", "[]"):
            assert t.count(a) == t.count(b), (path, a, t.count(a), t.count(b))
        assert t.lstrip().startswith("package " + package), path
    for path in OVERLAYS.values():
        assert '"github.com/ldsec/lattigo/ring"' in open(path).read()


def test_every_c_call_matches_the_header_and_the_encryptor_abi_is_reached():
    arity = _header_arity()
    t = _strip(open(SHIM).read())
    seen = set()
    for m in re.finditer(r"\bC\.(lr_[a-z0-9_]+)\s*\(", t):
        sym = m.group(1)
        assert sym in arity, (sym, "not declared in include/lattigo_ring.h")
        assert len(_call_args(t, m.end())) == arity[sym], (sym, arity[sym])
        seen.add(sym)
    abi = {s for s in arity if s.startswith(("lr_bfv_encryptor_", "lr_bfv_encrypt_", "lr_bfv_decryptor_", "lr_bfv_decrypt"))}
    assert len(abi) == 10 and abi <= seen, sorted(abi - seen)
    # the encoder's count (tests/test_go_bfv_encoder.py) is untouched by the new names
    assert not [s for s in abi if s.startswith(("lr_bfv_encoder_", "lr_bfv_encode_", "lr_bfv_decode_"))]


def test_go_1_13_language_level():
    for path in [SHIM] + list(OVERLAYS.values()):
        t = _strip(open(path).read())
        assert "runtime.Pinner" not in t and "unsafe.Slice" not in t and "unsafe.String" not in t, path
        assert not re.search(r"func \w+\[", t), (path, "type parameters")
        assert not re.search(r"\bany\b", t), path


def test_compact_samplers_run_the_upstream_samplers():
    text = open(SHIM).read()
    t = _strip(text)
    assert re.search(r"func \(kys \*KYSampler\) SampleCompact\(dst \[\]byte\)", t)
    assert re.search(r"func \(context \*Context\) SampleGaussianCompact\(dst \[\]byte, sigma float64, bound uint64\)", t)
    assert re.search(r"func SampleTernaryBits\(coeffs, signs \[\]byte\)", t)
    body = lambda name: t[t.index(name):].split("\nfunc ")[0]
    assert "kysampling(kys.Matrix, randomBytes, pointer)" in body("SampleCompact(dst") and "byte(sign)<<7" in body("SampleCompact(dst")
    assert "normFloat64(randomBytes)" in body("SampleGaussianCompact(dst") and "byte(sign)<<7" in body("SampleGaussianCompact(dst")
    assert body("func SampleTernaryBits").count("rand.Read(") == 2                     # two reads, the coefficient plane first
    assert '"crypto/rand"' in text


def test_overlays_call_what_the_shim_exports():
    shim = open(SHIM).read()
    enc, dec = _methods(shim, "BfvEncryptor"), _methods(shim, "BfvDecryptor")
    assert {"EncryptPk": 8, "EncryptSk": 6, "EncryptPkDevice": 8, "EncryptSkDevice": 6} == enc and dec == {"Decrypt": 3}
    assert re.search(r"func NewBfvEncryptor\(contextQ, contextP \*Context, maxBatch int\) \*BfvEncryptor", shim)
    assert re.search(r"func NewBfvDecryptor\(contextQ \*Context, maxBatch int\) \*BfvDecryptor", shim)
    samplers = {"SampleCompact": 1, "SampleGaussianCompact": 3, "SampleTernaryBits": 2}
    t = _strip(open(OVERLAYS["encryptor"]).read())
    calls = list(re.finditer(r"\.dev\(\)\.(\w+)\(", t))
    assert {m.group(1) for m in calls} == {"EncryptPk", "EncryptSk"}
    for m in calls:
        assert len(_call_args(t, m.end())) == enc[m.group(1)], m.group(1)
    for name, n in samplers.items():
        found = list(re.finditer(r"\b%s\(" % name, t))
        assert found, name
        for m in found:
            assert len(_call_args(t, m.end())) == n, name
    assert len(_call_args(t, re.search(r"ring\.NewBfvEncryptor\(", t).end())) == 3
    assert re.search(r"func \(\w+ \*encryptor\) dev\(\) \*ring\.BfvEncryptor", t)
    assert t.index("SampleTernaryBits(") < t.index("SampleCompact(e0)") < t.index("SampleCompact(e1)")       # upstream's order: u, e0, e1
    t = _strip(open(OVERLAYS["decryptor"]).read())
    calls = list(re.finditer(r"\.dev\(\)\.(\w+)\(", t))
    assert [m.group(1) for m in calls] == ["Decrypt"] and len(_call_args(t, calls[0].end())) == dec["Decrypt"]
    assert len(_call_args(t, re.search(r"ring\.NewBfvDecryptor\(", t).end())) == 2
    assert re.search(r"func \(\w+ \*decryptor\) dev\(\) \*ring\.BfvDecryptor", t)


def test_replacement_bodies_keep_the_upstream_signatures():
    ref = json.load(open(NAMES))
    up = ref["signatures"]
    helpers = {"dev", "ReleaseDevice"}
    mine = {}
    texts = {k: open(p).read() for k, p in OVERLAYS.items()}
    for text in texts.values():
        for m in re.finditer(r"func \(\w+ \*(\w+)\) (\w+)\(([^)]*)\)([^{]*)\{", text):
            params = re.sub(r"\s+", " ", m.group(3)).strip()
            types = [re.sub(r"^\w+ ", "", g.strip()) for g in _split_args(params)] if params else []
            mine[m.group(1) + "." + m.group(2)] = [types, re.sub(r"\s+", " ", m.group(4)).strip()]
    replaced = {k: v for k, v in mine.items() if k.split(".")[1] not in helpers}
    assert set(replaced) == set(up) == {"pkEncryptor.encrypt", "skEncryptor.encrypt", "decryptor.Decrypt"}
    for name, sig in replaced.items():
        assert sig == up[name], (name, sig, up[name])
    for name in helpers:
        for struct, fields in ref["fields"].items():
            assert name not in fields, (struct, name)
    enc, dec = texts["encryptor"], texts["decryptor"]
    assert re.search(r"delete\s+pkEncryptor\.encrypt\b", enc) and re.search(r"delete\s+skEncryptor\.encrypt\b", enc)
    assert re.search(r"delete\s+Decrypt\b", dec)
    both = enc + dec
    for ident in ref["upstream_identifiers_found"]:
        assert ident in both, ident
    # every field the overlays read through their receivers exists upstream (embedded structs included) or is one of their helpers
    for field in re.findall(r"\bencryptor\.(\w+)", _strip(enc)):
        assert field in ref["fields"]["encryptor"] + ref["fields"]["pkEncryptor"] + ref["fields"]["skEncryptor"] or field in helpers, field
    for field in re.findall(r"\bdecryptor\.(\w+)", _strip(dec)):
        assert field in ref["fields"]["decryptor"] or field in helpers, field
