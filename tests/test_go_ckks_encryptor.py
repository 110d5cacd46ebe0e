"""The CKKS encryptor's Go side cannot be compiled here (no Go toolchain in the image): go/ring/ckks_encryptor.go (the cgo type CkksEncryptor;
the compact samplers are those of go/ring/bfv_encryptor.go) and go/ckks/encryptor_device.go, go/ckks/decryptor_device.go (replacement bodies for
pkEncryptor.encrypt, skEncryptor.encrypt and decryptor.Decrypt) are checked statically, in the manner of test_go_bfv_encryptor.py -- every C
symbol called is declared in include/lattigo_ring.h with the same number of arguments and every lr_ckks_encryptor_* symbol of the header is
reached, delimiters balance, the go 1.13 language level holds, the overlays call only what the shim has, with its arity, and their methods
keep the upstream signatures (tests/golden/reference_ckks_encryptor_names.json)."""
import json
import os
import re

from conftest import ROOT
from test_go_bfv_encoder import _call_args
from test_go_bfv_encryptor import _methods
from test_go_shim import _header_arity, _split_args, _strip

SHIM = os.path.join(ROOT, "go", "ring", "ckks_encryptor.go")
SAMPLERS = os.path.join(ROOT, "go", "ring", "bfv_encryptor.go")
PIPELINES = os.path.join(ROOT, "go", "ring", "pipelines.go")
OVERLAYS = {"encryptor": os.path.join(ROOT, "go", "ckks", "encryptor_device.go"), "decryptor": os.path.join(ROOT, "go", "ckks", "decryptor_device.go")}
NAMES = os.path.join(ROOT, "tests", "golden", "reference_ckks_encryptor_names.json")


def test_delimiters_balance_and_packages():
    for path, package in [(SHIM, "ring")] + [(p, "ckks") for p in OVERLAYS.values()]:
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
    abi = {s for s in arity if s.startswith("lr_ckks_encryptor_")}
    assert len(abi) == 7 and abi == seen, sorted(abi ^ seen)
    # every call passes the level right behind the form, as the header declares it
    for m in re.finditer(r"\bC\.lr_ckks_encryptor_encrypt_\w+\s*\(", t):
        args = [a.strip() for a in _call_args(t, m.end())]
        assert args[1] == "cBool(fast)" and args[2] == "C.int(level)", args[:3]


def test_go_1_13_language_level():
    for path in [SHIM] + list(OVERLAYS.values()):
        t = _strip(open(path).read())
        assert "runtime.Pinner" not in t and "unsafe.Slice" not in t and "unsafe.String" not in t, path
        assert not re.search(r"func \w+\[", t), (path, "type parameters")
        assert not re.search(r"\bany\b", t), path


def test_the_shim_reuses_the_exported_samplers():
    """one set of decision recorders for both schemes: the shim defines none of its own and needs bytePtr / cBool from its package"""
    t, samplers = _strip(open(SHIM).read()), _strip(open(SAMPLERS).read())
    for name in ("SampleCompact", "SampleGaussianCompact", "SampleTernaryBits", "bytePtr"):
        assert not re.search(r"func (\([^)]*\) )?%s\(" % name, t), name
        assert re.search(r"func (\([^)]*\) )?%s\(" % name, samplers), name
    assert "crypto/rand" not in open(SHIM).read()


def test_overlays_call_what_the_shim_exports():
    shim = open(SHIM).read()
    enc = _methods(shim, "CkksEncryptor")
    assert {"EncryptPk": 9, "EncryptSk": 7, "EncryptPkDevice": 9, "EncryptSkDevice": 7} == enc
    assert re.search(r"func NewCkksEncryptor\(contextQ, contextP \*Context, maxBatch int\) \*CkksEncryptor", shim)
    plan = _methods(open(PIPELINES).read(), "CkksPlan")
    assert plan["Decrypt"] == 4
    samplers = {"SampleCompact": 1, "SampleTernaryBits": 2}
    t = _strip(open(OVERLAYS["encryptor"]).read())
    calls = list(re.finditer(r"\.dev\(\)\.(\w+)\(", t))
    assert {m.group(1) for m in calls} == {"EncryptPk", "EncryptSk"}
    for m in calls:
        args = _call_args(t, m.end())
        assert len(args) == enc[m.group(1)], m.group(1)
        assert args[0].strip() == "plaintext.Level()" and args[-1].strip() == "fast", m.group(1)
    for name, n in samplers.items():
        found = list(re.finditer(r"\b%s\(" % name, t))
        assert found, name
        for m in found:
            assert len(_call_args(t, m.end())) == n, name
    assert len(_call_args(t, re.search(r"ring\.NewCkksEncryptor\(", t).end())) == 3
    assert re.search(r"func \(\w+ \*encryptor\) dev\(\) \*ring\.CkksEncryptor", t)
    assert t.index("SampleTernaryBits(") < t.index("SampleCompact(e0)") < t.index("SampleCompact(e1)")       # upstream's order: u, e0, e1
    assert t.count("ciphertext.isNTT = true") == 2                                                           # :236, :361
    t = _strip(open(OVERLAYS["decryptor"]).read())
    calls = list(re.finditer(r"\.dev\(\)\.(\w+)\(", t))
    assert [m.group(1) for m in calls] == ["Decrypt"] and len(_call_args(t, calls[0].end())) == plan["Decrypt"]
    assert len(_call_args(t, re.search(r"ring\.NewCkksPlan\(", t).end())) == 3
    assert re.search(r"func \(\w+ \*decryptor\) dev\(\) \*ring\.CkksPlan", t)


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
    # the eight interface methods stay upstream's and are named as kept: each ends in one of the two bodies
    assert len(ref["interface_methods"]) == 8
    for name in ref["interface_methods"]:
        assert re.search(r"\b%s\b" % name, enc), name
        assert not re.search(r"func \(\w+ \*\w+\) %s\(" % name, enc), (name, "defined twice once the overlay is added")
    both = enc + dec
    for ident in ref["upstream_identifiers_found"]:
        assert ident in both, ident
    # every field the overlays read through their receivers exists upstream (embedded structs included) or is one of their helpers
    for field in re.findall(r"\bencryptor\.(\w+)", _strip(enc)):
        assert field in ref["fields"]["encryptor"] + ref["fields"]["pkEncryptor"] + ref["fields"]["skEncryptor"] or field in helpers, field
    for field in re.findall(r"\bdecryptor\.(\w+)", _strip(dec)):
        assert field in ref["fields"]["decryptor"] or field in helpers, field
