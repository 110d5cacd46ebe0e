"""The CKKS encoder's Go side cannot be compiled here (no Go toolchain in the image): go/ring/ckks_encoder.go (the cgo type CkksEncoder) and
go/ckks/encoder_device.go (replacement bodies for Encode and Decode of the upstream *encoder) are checked statically with the helpers of
test_go_bfv_encoder.py -- every C symbol called is declared in include/lattigo_ring.h with the same number of arguments and every
lr_ckks_encoder_* / lr_ckks_encode* / lr_ckks_decode* symbol of the header is reached, delimiters balance, the go 1.13 language level holds,
the overlay calls only methods CkksEncoder has, with their arity, passes the reference's root table, level and scale, and its methods keep
the upstream signatures (tests/golden/reference_ckks_encoder_names.json)."""
import json
import os
import re

from conftest import ROOT
from test_go_bfv_encoder import _call_args
from test_go_shim import _header_arity, _split_args, _strip

SHIM = os.path.join(ROOT, "go", "ring", "ckks_encoder.go")
OVERLAY = os.path.join(ROOT, "go", "ckks", "encoder_device.go")
NAMES = os.path.join(ROOT, "tests", "golden", "reference_ckks_encoder_names.json")
PREFIXES = ("lr_ckks_encoder_", "lr_ckks_encode", "lr_ckks_decode")


def test_delimiters_balance_and_packages():
    for path, package in ((SHIM, "ring"), (OVERLAY, "ckks")):
        t = _strip(open(path).read())
        for a, b in ("{}", "()", "[]"):
            assert t.count(a) == t.count(b), (path, a, t.count(a), t.count(b))
        assert t.lstrip().startswith("package " + package), path
    assert '"github.com/ldsec/lattigo/ring"' in open(OVERLAY).read()


def test_every_c_call_matches_the_header_and_the_encoder_abi_is_reached():
    arity = _header_arity()
    t = _strip(open(SHIM).read())
    seen = set()
    for m in re.finditer(r"\bC\.(lr_[a-z0-9_]+)\s*\(", t):
        sym = m.group(1)
        assert sym in arity, (sym, "not declared in include/lattigo_ring.h")
        assert len(_call_args(t, m.end())) == arity[sym], (sym, arity[sym])
        seen.add(sym)
    abi = {s for s in arity if s.startswith(PREFIXES)}
    assert len(abi) == 9 and abi <= seen, sorted(abi - seen)
    # the new symbols stay clear of the BFV encoder's prefixes, which test_go_bfv_encoder.py counts
    assert not any(s.startswith(("lr_bfv_encoder_", "lr_bfv_encode_", "lr_bfv_decode_")) for s in abi)


def test_the_option_field_is_settable_from_go():
    header = open(os.path.join(ROOT, "include", "lattigo_ring.h")).read()
    options = open(os.path.join(ROOT, "go", "ring", "options.go")).read()
    assert re.search(r"int32_t\s+ckks_encoder_tiled;", header)
    assert 'case "ckks_encoder_tiled":' in options and "o.c.ckks_encoder_tiled = C.int32_t(value)" in options


def test_go_1_13_language_level():
    for path in (SHIM, OVERLAY):
        t = _strip(open(path).read())
        assert "runtime.Pinner" not in t and "unsafe.Slice" not in t and "unsafe.String" not in t, path
        assert not re.search(r"func \w+\[", t), (path, "type parameters")
        assert not re.search(r"\bany\b", t), path


def test_overlay_calls_what_the_shim_exports():
    shim = open(SHIM).read()
    methods = {m.group(1): len([g for g in _split_args(m.group(2)) if g.strip()])
               for m in re.finditer(r"func \(\w+ \*CkksEncoder\) (\w+)\(([^)]*)\)", shim)}
    assert {"Encode", "Decode", "Tables", "Fused", "EncodeDevice", "DecodeDevice"} <= set(methods)
    assert re.search(r"func NewCkksEncoder\(contextQ \*Context, maxBatch int, roots \[\]complex128\) \*CkksEncoder", shim)
    t = _strip(open(OVERLAY).read())
    calls = list(re.finditer(r"\.dev\(\)\.(\w+)\(", t))
    assert {m.group(1) for m in calls} == {"Encode", "Decode"}
    for m in calls:
        args = _call_args(t, m.end())
        assert len(args) == methods[m.group(1)], m.group(1)
        # the level and the scale of the plaintext at hand, not the parameters' maxima
        assert [a.strip() for a in args[-2:]] == ["plaintext.Level()", "plaintext.scale"], m.group(1)
    create = _call_args(t, re.search(r"ring\.NewCkksEncoder\(", t).end())
    assert len(create) == 3 and create[2].strip() == "encoder.roots"
    assert re.search(r"func \(\w+ \*encoder\) dev\(\) \*ring\.CkksEncoder", t)


def test_replacement_bodies_keep_the_upstream_signatures():
    ref = json.load(open(NAMES))
    up = ref["encoder_signatures"]
    text = open(OVERLAY).read()
    mine = {}
    for m in re.finditer(r"func \(encoder \*encoder\) (\w+)\(([^)]*)\)([^{]*)\{", text):
        params = re.sub(r"\s+", " ", m.group(2)).strip()
        types = [re.sub(r"^\w+ ", "", g.strip()) for g in _split_args(params)] if params else []
        mine[m.group(1)] = [types, re.sub(r"\s+", " ", m.group(3)).strip()]
    helpers = {"dev", "ReleaseDevice"}
    assert set(mine) - helpers == {"Encode", "Decode"}
    for name, (types, ret) in mine.items():
        if name in helpers:
            assert name not in up and name not in ref["encoder_fields"], name
            continue
        assert [types, ret] == up[name], (name, types, ret, up[name])
        assert re.search(r"delete\s+%s\b" % name, text), (name, "missing from the patch list in the header")
    for gone in ("invfftlazy", "invfft", "fft"):
        assert re.search(r"\b%s\b" % gone, text.split("package ckks")[0]), gone
    for ident in ref["upstream_identifiers_found"]:
        assert ident in text, ident
    for field in re.findall(r"encoder\.(\w+)", _strip(text)):
        assert field in ref["encoder_fields"] or field in mine, field
