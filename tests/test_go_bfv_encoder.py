"""The BFV encoder's Go side cannot be compiled here (no Go toolchain in the image): go/ring/bfv_encoder.go (the cgo type BfvEncoder) and
go/bfv/encoder_device.go (replacement bodies for the four methods of the upstream *encoder) are checked statically, in the manner of
test_go_shim.py -- every C symbol called is declared in include/lattigo_ring.h with the same number of arguments and every lr_bfv_encode* /
lr_bfv_decode* / lr_bfv_encoder_* symbol of the header is reached, delimiters balance, the go 1.13 language level holds, the overlay calls
only methods BfvEncoder has, with their arity, and its methods keep the upstream signatures (tests/golden/reference_bfv_encoder_names.json)."""
import json
import os
import re

from conftest import ROOT
from test_go_shim import _header_arity, _split_args, _strip

SHIM = os.path.join(ROOT, "go", "ring", "bfv_encoder.go")
OVERLAY = os.path.join(ROOT, "go", "bfv", "encoder_device.go")
NAMES = os.path.join(ROOT, "tests", "golden", "reference_bfv_encoder_names.json")


def _call_args(t, end):
    i, depth = end, 1
    while depth:
        depth += {"(": 1, ")": -1}.get(t[i], 0)
        i += 1
    return _split_args(t[end:i - 1])


def test_delimiters_balance_and_packages():
    for path, package in ((SHIM, "ring"), (OVERLAY, "bfv")):
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
    abi = {s for s in arity if s.startswith(("lr_bfv_encoder_", "lr_bfv_encode_", "lr_bfv_decode_"))}
    assert len(abi) == 11 and abi <= seen, sorted(abi - seen)


def test_go_1_13_language_level():
    for path in (SHIM, OVERLAY):
        t = _strip(open(path).read())
        assert "runtime.Pinner" not in t and "unsafe.Slice" not in t and "unsafe.String" not in t, path
        assert not re.search(r"func \w+\[", t), (path, "type parameters")
        assert not re.search(r"\bany\b", t), path


def test_overlay_calls_what_the_shim_exports():
    shim = open(SHIM).read()
    methods = {m.group(1): len([g for g in _split_args(m.group(2)) if g.strip()])
               for m in re.finditer(r"func \(\w+ \*BfvEncoder\) (\w+)\(([^)]*)\)", shim)}
    assert {"EncodeUint", "EncodeInt", "DecodeUint", "DecodeInt", "Tables", "Fused", "EncodeDevice", "DecodeDevice"} <= set(methods)
    assert re.search(r"func NewBfvEncoder\(contextQ \*Context, t uint64, maxBatch int\) \*BfvEncoder", shim)
    t = _strip(open(OVERLAY).read())
    calls = list(re.finditer(r"\.dev\(\)\.(\w+)\(", t))
    assert {m.group(1) for m in calls} == {"EncodeUint", "EncodeInt", "DecodeUint", "DecodeInt"}
    for m in calls:
        assert len(_call_args(t, m.end())) == methods[m.group(1)], m.group(1)
    assert len(_call_args(t, re.search(r"ring\.NewBfvEncoder\(", t).end())) == 3
    assert re.search(r"func \(\w+ \*encoder\) dev\(\) \*ring\.BfvEncoder", t)


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
    assert set(mine) - helpers == {"EncodeUint", "EncodeInt", "DecodeUint", "DecodeInt"}
    for name, (types, ret) in mine.items():
        if name in helpers:
            assert name not in up and name not in ref["encoder_fields"], name
            continue
        assert [types, ret] == up[name], (name, types, ret, up[name])
        assert re.search(r"delete\s+%s\b" % name, text), (name, "missing from the patch list in the header")
    assert re.search(r"delete\s+encodePlaintext\b", text)
    for ident in ref["upstream_identifiers_found"]:
        assert ident in text, ident
    for field in re.findall(r"encoder\.(\w+)", _strip(text)):
        assert field in ref["encoder_fields"] or field in mine, field
