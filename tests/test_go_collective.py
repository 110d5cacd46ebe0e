"""The Go side of collective key switching cannot be compiled here (no Go toolchain in the image): go/ring/collective.go (the cgo type
Collective; the compact samplers are those of go/ring/bfv_encryptor.go) and the four overlays go/dckks/keyswitching_device.go,
go/dckks/public_keyswitching_device.go, go/dbfv/keyswitching_device.go, go/dbfv/public_keyswitching_device.go (replacement bodies for
GenShare, genShareDelta, AggregateShares and KeySwitch) are checked statically, in the manner of test_go_keygen.py -- every C symbol called
is declared in include/lattigo_ring.h with the same number of arguments and every lr_collective_* symbol of the header is reached,
delimiters balance, the go 1.13 language level holds, the overlays call only what the shim has, with its arity, and their methods keep the
upstream signatures (tests/golden/reference_collective_names.json)."""
import json
import os
import re

from conftest import ROOT
from test_go_bfv_encoder import _call_args
from test_go_bfv_encryptor import _methods
from test_go_shim import _header_arity, _split_args, _strip

SHIM = os.path.join(ROOT, "go", "ring", "collective.go")
SAMPLERS = os.path.join(ROOT, "go", "ring", "bfv_encryptor.go")
OVERLAYS = {("dckks", "CKSProtocol"): os.path.join(ROOT, "go", "dckks", "keyswitching_device.go"),
            ("dckks", "PCKSProtocol"): os.path.join(ROOT, "go", "dckks", "public_keyswitching_device.go"),
            ("dbfv", "CKSProtocol"): os.path.join(ROOT, "go", "dbfv", "keyswitching_device.go"),
            ("dbfv", "PCKSProtocol"): os.path.join(ROOT, "go", "dbfv", "public_keyswitching_device.go")}
NAMES = os.path.join(ROOT, "tests", "golden", "reference_collective_names.json")
REPLACED = {"CKSProtocol": {"GenShare", "genShareDelta", "AggregateShares", "KeySwitch"}, "PCKSProtocol": {"GenShare", "AggregateShares", "KeySwitch"}}
HELPERS = {"dev", "ReleaseDevice", "top"}
SHARE_CALL = {("dckks", "CKSProtocol"): "CkksCksShare", ("dckks", "PCKSProtocol"): "CkksPcksShare", ("dbfv", "CKSProtocol"): "BfvCksShare",
              ("dbfv", "PCKSProtocol"): "BfvPcksShare"}


def test_delimiters_balance_and_packages():
    for path, package in [(SHIM, "ring")] + [(p, k[0]) for k, p in OVERLAYS.items()]:
        t = _strip(open(path).read())
        for a, b in ("{}", "()", "[]"):
            assert t.count(a) == t.count(b), (path, a, t.count(a), t.count(b))
        assert t.lstrip().startswith("package " + package), path
    for (pkg, _), path in OVERLAYS.items():
        text = open(path).read()
        assert '"github.com/ldsec/lattigo/ring"' in text and '"github.com/ldsec/lattigo/%s"' % pkg[1:] in text, path


def test_every_c_call_matches_the_header_and_the_collective_abi_is_reached():
    arity = _header_arity()
    t = _strip(open(SHIM).read())
    seen = set()
    for m in re.finditer(r"\bC\.(lr_[a-z0-9_]+)\s*\(", t):
        sym = m.group(1)
        assert sym in arity, (sym, "not declared in include/lattigo_ring.h")
        assert len(_call_args(t, m.end())) == arity[sym], (sym, arity[sym])
        seen.add(sym)
    abi = {s for s in arity if s.startswith("lr_collective_")}
    assert len(abi) == 12 and abi == seen, sorted(abi ^ seen)
    # the CKKS calls pass the level right behind the handle, as the header declares it; the fold hands over the count of its shares
    for m in re.finditer(r"\bC\.lr_collective_ckks_\w+\s*\(", t):
        assert [a.strip() for a in _call_args(t, m.end())][1] == "C.int(level)"
    args = [a.strip() for a in _call_args(t, re.search(r"\bC\.lr_collective_aggregate\s*\(", t).end())]
    assert args[1] == "C.int(level)" and args[4] == "C.int(n)" and "n := len(shares)" in t


def test_go_1_13_language_level():
    for path in [SHIM] + list(OVERLAYS.values()):
        t = _strip(open(path).read())
        assert "runtime.Pinner" not in t and "unsafe.Slice" not in t and "unsafe.String" not in t, path
        assert not re.search(r"func \w+\[", t), (path, "type parameters")
        assert not re.search(r"\bany\b", t), path


def test_the_shim_reuses_the_exported_samplers():
    """one set of decision recorders for every handle: the shim defines none of its own and needs bytePtr / polyArray from its package"""
    t, samplers = _strip(open(SHIM).read()), _strip(open(SAMPLERS).read())
    for name in ("SampleCompact", "SampleGaussianCompact", "SampleTernaryBits", "bytePtr"):
        assert not re.search(r"func (\([^)]*\) )?%s\(" % name, t), name
        assert re.search(r"func (\([^)]*\) )?%s\(" % name, samplers), name
    assert "crypto/rand" not in open(SHIM).read()
    assert "func polyArray(" in open(os.path.join(ROOT, "go", "ring", "pipelines.go")).read()


def test_overlays_call_what_the_shim_exports():
    shim = open(SHIM).read()
    col = _methods(shim, "Collective")
    assert {"CkksCksShare": 6, "BfvCksShare": 5, "CkksPcksShare": 9, "BfvPcksShare": 8, "Aggregate": 4}.items() <= col.items()
    for name in ("CkksCksShare", "BfvCksShare", "CkksPcksShare", "BfvPcksShare"):
        assert col[name + "Device"] == col[name] + 1, name            # the batch
    assert re.search(r"func NewCollective\(contextQ, contextP \*Context, maxBatch int\) \*Collective", shim)
    for key, path in OVERLAYS.items():
        pkg, proto = key
        t = _strip(open(path).read())
        calls = list(re.finditer(r"\.dev\(\)\.(\w+)\(", t))
        assert {m.group(1) for m in calls} == {SHARE_CALL[key], "Aggregate"}, key
        for m in calls:
            assert len(_call_args(t, m.end())) == col[m.group(1)], (key, m.group(1))
        assert len(_call_args(t, re.search(r"ring\.NewCollective\(", t).end())) == 3
        assert re.search(r"func \(\w+ \*%s\) dev\(\) \*ring\.Collective" % proto, t)
        assert re.search(r"func \(\w+ \*%s\) ReleaseDevice\(\)" % proto, t) and "Protocols.Delete(" in t
        # the samplers in upstream's order: u, then the smudging sampler's e0, then the regular sampler's e1
        body = t[t.index(") GenShare("):]
        if proto == "PCKSProtocol":
            assert body.index("SampleTernaryBits(") < body.index("gaussianSamplerSmudge.SampleCompact(e0)") < body.index("gaussianSampler.SampleCompact(e1)")
            assert len(re.findall(r"\bSampleCompact\(", t)) == 2
        else:
            assert len(re.findall(r"gaussianSamplerSmudge\.SampleCompact\(noise\)", t)) == 2      # GenShare and genShareDelta
        # KeySwitch: the Add onto ct[0], then the Copy -- two folds; AggregateShares: one fold per component
        ks = t[t.index(") KeySwitch("):]
        assert ks.count(".dev().Aggregate(") == 2 and "ct.Value()[0], []*ring.Poly{" in ks and ", nil, []*ring.Poly{" in ks
        if pkg == "dckks":
            assert "ctOut.SetScale(ct.Scale())" in ks


def test_replacement_bodies_keep_the_upstream_signatures():
    ref = json.load(open(NAMES))
    for (pkg, proto), path in OVERLAYS.items():
        up, text = ref["signatures"][pkg][proto], open(path).read()
        mine = {}
        for m in re.finditer(r"func \(\w+ \*%s\) (\w+)\(([^)]*)\)([^{]*)\{" % proto, text):
            params = re.sub(r"\s+", " ", m.group(2)).strip()
            types = [re.sub(r"^\w+ ", "", g.strip()) if " " in g.strip() else None for g in _split_args(params)] if params else []
            for i in range(len(types) - 2, -1, -1):
                if types[i] is None:
                    types[i] = types[i + 1]
            mine[m.group(1)] = [types, re.sub(r"\s+", " ", m.group(3)).strip()]
        replaced = {k: v for k, v in mine.items() if k not in HELPERS}
        assert set(replaced) == REPLACED[proto], (pkg, proto, sorted(replaced))
        for name, sig in replaced.items():
            assert sig == up[name], (pkg, proto, name, sig, up[name])
            assert re.search(r"delete\s+%s\b" % name, text), (pkg, proto, name, "missing from the patch list in the header")
        for name in HELPERS:
            assert name not in up and name not in ref["fields"][pkg][proto], (pkg, proto, name)
        # what stays upstream's is named as kept and not defined twice
        for name in set(up) - REPLACED[proto]:
            assert name in text and not re.search(r"func \(\w+ \*%s\) %s\(" % (proto, name), text), (pkg, proto, name)
        # every field the overlay reads through its receiver or its context exists upstream
        t = _strip(text)
        ctx = "dckksContext" if pkg == "dckks" else "dbfvContext"
        recv = "cks" if proto == "CKSProtocol" else "pcks"
        for field in re.findall(r"\b%s\.(\w+)" % recv, t):
            assert field in ref["fields"][pkg][proto] or field in HELPERS, (pkg, proto, field)
        for field in re.findall(r"\b%s\.(?:dckksContext|context)\.(\w+)" % recv, t):
            assert field in ref["fields"][pkg][ctx], (pkg, proto, field)
        for ident in ("contextQ", "contextP", "gaussianSamplerSmudge", "ct.Value()", "CKSShare" if proto == "CKSProtocol" else "PCKSShare"):
            assert ident in ref["upstream_identifiers_found"][pkg] and ident in text, (pkg, proto, ident)
