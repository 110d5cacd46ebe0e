"""The Go side of the collective Refresh cannot be compiled here (no Go toolchain in the image): go/ring/refresh.go (the cgo type Refresh;
the compact samplers are those of go/ring/bfv_encryptor.go) and the two overlays go/dckks/public_refresh_device.go and
go/dbfv/public_refresh_device.go (replacement bodies for GenShares, Aggregate, Decrypt and dckks's Recode / Recrypt, dbfv's Finalize) are
checked statically, in the manner of test_go_collective.py -- every C symbol called is declared in include/lattigo_ring.h with the same
number of arguments and every lr_refresh_* symbol of the header is reached, delimiters balance, the go 1.13 language level holds, the
overlays call only what the shim has, with its arity, and their methods keep the upstream signatures
(tests/golden/reference_refresh_names.json)."""
import json
import os
import re

from conftest import ROOT
from test_go_bfv_encoder import _call_args
from test_go_bfv_encryptor import _methods
from test_go_shim import _header_arity, _split_args, _strip

SHIM = os.path.join(ROOT, "go", "ring", "refresh.go")
SAMPLERS = os.path.join(ROOT, "go", "ring", "bfv_encryptor.go")
OVERLAYS = {"dckks": os.path.join(ROOT, "go", "dckks", "public_refresh_device.go"), "dbfv": os.path.join(ROOT, "go", "dbfv", "public_refresh_device.go")}
NAMES = os.path.join(ROOT, "tests", "golden", "reference_refresh_names.json")
REPLACED = {"dckks": {"GenShares", "Aggregate", "Decrypt", "Recode", "Recrypt"}, "dbfv": {"GenShares", "Aggregate", "Decrypt", "Finalize"}}
HELPERS = {"dev", "ReleaseDevice", "top"}
CALLS = {"dckks": {"CkksGenShares", "CkksRecode", "Aggregate", "MaskWords"}, "dbfv": {"BfvGenShares", "BfvFinalize", "Aggregate"}}


def test_delimiters_balance_and_packages():
    for path, package in [(SHIM, "ring")] + [(p, k) for k, p in OVERLAYS.items()]:
        t = _strip(open(path).read())
        for a, b in ("{}", "()", "[]"):
            assert t.count(a) == t.count(b), (path, a, t.count(a), t.count(b))
        assert t.lstrip().startswith("package " + package), path
    for pkg, path in OVERLAYS.items():
        text = open(path).read()
        assert '"github.com/ldsec/lattigo/ring"' in text and '"github.com/ldsec/lattigo/%s"' % pkg[1:] in text, path


def test_every_c_call_matches_the_header_and_the_refresh_abi_is_reached():
    arity = _header_arity()
    t = _strip(open(SHIM).read())
    seen = set()
    for m in re.finditer(r"\bC\.(lr_[a-z0-9_]+)\s*\(", t):
        sym = m.group(1)
        assert sym in arity, (sym, "not declared in include/lattigo_ring.h")
        assert len(_call_args(t, m.end())) == arity[sym], (sym, arity[sym])
        seen.add(sym)
    abi = {s for s in arity if s.startswith("lr_refresh_")}
    assert len(abi) == 12 and abi == seen, sorted(abi ^ seen)
    # the CKKS calls pass levelStart right behind the handle, as the header declares it; the fold hands over the count of its shares
    for m in re.finditer(r"\bC\.lr_refresh_ckks_\w+\s*\(", t):
        assert [a.strip() for a in _call_args(t, m.end())][1] == "C.int(levelStart)"
    args = [a.strip() for a in _call_args(t, re.search(r"\bC\.lr_refresh_aggregate\s*\(", t).end())]
    assert args[1] == "C.int(level)" and args[3] == "C.int(n)" and "n := len(shares)" in t
    # the host forms make one pair of shares per call; the Device forms pass the caller's batch
    for name in ("ckks_shares", "bfv_shares"):
        host = [a.strip() for a in _call_args(t, re.search(r"\bC\.lr_refresh_%s\s*\(" % name, t).end())]
        dev = [a.strip() for a in _call_args(t, re.search(r"\bC\.lr_refresh_%s_device\s*\(" % name, t).end())]
        assert host[-3] == "1" and dev[-3] == "C.int(batch)", name


def test_go_1_13_language_level():
    for path in [SHIM] + list(OVERLAYS.values()):
        t = _strip(open(path).read())
        assert "runtime.Pinner" not in t and "unsafe.Slice" not in t and "unsafe.String" not in t, path
        assert not re.search(r"func \w+\[", t), (path, "type parameters")
        assert not re.search(r"\bany\b", t), path


def test_the_shim_reuses_the_exported_samplers():
    t, samplers = _strip(open(SHIM).read()), _strip(open(SAMPLERS).read())
    for name in ("SampleCompact", "SampleGaussianCompact", "SampleTernaryBits", "bytePtr"):
        assert not re.search(r"func (\([^)]*\) )?%s\(" % name, t), name
        assert re.search(r"func (\([^)]*\) )?%s\(" % name, samplers), name
    assert "crypto/rand" not in open(SHIM).read()
    assert "func polyArray(" in open(os.path.join(ROOT, "go", "ring", "pipelines.go")).read()
    # the word planes: word k of coefficient j at k n + j, negative values through 2^(64 words)
    assert "planes[k*n+j]" in open(SHIM).read() and "Lsh(big.NewInt(1), uint(64*words))" in open(SHIM).read()


def test_overlays_call_what_the_shim_exports():
    shim = open(SHIM).read()
    ref = _methods(shim, "Refresh")
    assert {"MaskWords": 1, "CkksGenShares": 9, "CkksRecode": 3, "CkksFinalize": 5, "BfvGenShares": 8, "BfvFinalize": 6, "Aggregate": 3}.items() <= ref.items()
    for name in ("CkksGenShares", "BfvGenShares"):
        assert ref[name + "Device"] == ref[name] + 1, name            # the batch
    assert re.search(r"func NewRefresh\(contextQ, contextP \*Context, t uint64, maxBatch int\) \*Refresh", shim)
    assert re.search(r"func MaskWordPlanes\(mask \[\]\*big\.Int, words int\) \[\]uint64", shim)
    for pkg, path in OVERLAYS.items():
        t = _strip(open(path).read())
        calls = list(re.finditer(r"\.dev\(\)\.(\w+)\(", t))
        assert {m.group(1) for m in calls} == CALLS[pkg], pkg
        for m in calls:
            assert len(_call_args(t, m.end())) == ref[m.group(1)], (pkg, m.group(1))
        assert len(_call_args(t, re.search(r"ring\.NewRefresh\(", t).end())) == 4
        assert re.search(r"func \(\w+ \*RefreshProtocol\) dev\(\) \*ring\.Refresh", t)
        assert re.search(r"func \(\w+ \*RefreshProtocol\) ReleaseDevice\(\)", t) and "Protocols.Delete(" in t
        # the samplers in upstream's order: e0 of the decryption share, then e1 of the recryption share
        body = t[t.index(") GenShares("):]
        assert body.index("gaussianSampler.SampleCompact(e0)") < body.index("gaussianSampler.SampleCompact(e1)")
        assert len(re.findall(r"\bSampleCompact\(", t)) == 2
    dckks = _strip(open(OVERLAYS["dckks"]).read())
    assert "ring.MaskWordPlanes(refreshProtocol.maskBigint, refreshProtocol.dev().MaskWords(levelStart))" in dckks
    assert "m.Cmp(half) >= 0" in dckks                                  # upstream's sign == 1 || sign == 0
    assert "ciphertext.Value()[1] = crs.CopyNew()" in dckks[dckks.index(") Recrypt("):]
    assert "accumulates unreduced noise" in open(OVERLAYS["dbfv"]).read() and "accumulates unreduced noise" in shim


def test_replacement_bodies_keep_the_upstream_signatures():
    ref = json.load(open(NAMES))
    for pkg, path in OVERLAYS.items():
        up, text = ref["signatures"][pkg]["RefreshProtocol"], open(path).read()
        mine = {}
        for m in re.finditer(r"func \(\w+ \*RefreshProtocol\) (\w+)\(([^)]*)\)([^{]*)\{", text):
            params = re.sub(r"\s+", " ", m.group(2)).strip()
            types = [re.sub(r"^\w+ ", "", g.strip()) if " " in g.strip() else None for g in _split_args(params)] if params else []
            for i in range(len(types) - 2, -1, -1):
                if types[i] is None:
                    types[i] = types[i + 1]
            mine[m.group(1)] = [types, re.sub(r"\s+", " ", m.group(3)).strip()]
        replaced = {k: v for k, v in mine.items() if k not in HELPERS}
        assert set(replaced) == REPLACED[pkg], (pkg, sorted(replaced))
        for name, sig in replaced.items():
            assert sig == up[name], (pkg, name, sig, up[name])
            assert re.search(r"delete\s+%s\b" % name, text), (pkg, name, "missing from the patch list in the header")
        for name in HELPERS:
            assert name not in up and name not in ref["fields"][pkg]["RefreshProtocol"], (pkg, name)
        # what stays upstream's is named as kept and not defined twice
        for name in set(up) - REPLACED[pkg]:
            assert name in text and not re.search(r"func \(\w+ \*RefreshProtocol\) %s\(" % name, text), (pkg, name)
        # every field the overlay reads through its receiver or its context exists upstream
        t = _strip(text)
        ctx, recv = ("dckksContext", "refreshProtocol") if pkg == "dckks" else ("dbfvContext", "rfp")
        for field in re.findall(r"\b%s\.(\w+)" % recv, t):
            assert field in ref["fields"][pkg]["RefreshProtocol"] or field in HELPERS, (pkg, field)
        for field in re.findall(r"\b%s\.(?:dckksContext|context)\.(\w+)" % recv, t):
            assert field in ref["fields"][pkg][ctx], (pkg, field)
        for ident in ("contextQ", "gaussianSampler", "ciphertext.Value()", "RefreshShareDecrypt", "RefreshShareRecrypt"):
            assert ident in ref["upstream_identifiers_found"][pkg] and ident in text, (pkg, ident)
