"""The Go side of the collective key setup cannot be compiled here (no Go toolchain in the image): go/ring/setup.go (the cgo type Setup; the
compact samplers are those of go/ring/bfv_encryptor.go) and the eight overlays publickey_gen_device.go, relinkey_gen_device.go,
relinkey_gen_naive_device.go and rotkey_gen_device.go of go/dbfv and go/dckks (replacement bodies for the GenShare*, Aggregate* and
finalize methods of CKGProtocol, RKGProtocol, RKGProtocolNaive and RTGProtocol) are checked statically, in the manner of
test_go_collective.py -- every C symbol called is declared in include/lattigo_ring.h with the same number of arguments and every
lr_setup_* symbol of the header is reached, delimiters balance, the go 1.13 language level holds, the overlays call only what the shim
has, with its arity, their methods keep the upstream signatures and read only upstream's fields
(tests/golden/reference_setup_names.json), and the samplers are called in upstream's order."""
import json
import os
import re

from conftest import ROOT
from test_go_bfv_encoder import _call_args
from test_go_bfv_encryptor import _methods
from test_go_shim import _header_arity, _split_args, _strip

SHIM = os.path.join(ROOT, "go", "ring", "setup.go")
SAMPLERS = os.path.join(ROOT, "go", "ring", "bfv_encryptor.go")
FILES = {"CKGProtocol": "publickey_gen_device.go", "RKGProtocol": "relinkey_gen_device.go", "RKGProtocolNaive": "relinkey_gen_naive_device.go",
         "RTGProtocol": "rotkey_gen_device.go"}
OVERLAYS = {(pkg, proto): os.path.join(ROOT, "go", pkg, f) for pkg in ("dbfv", "dckks") for proto, f in FILES.items()}
NAMES = os.path.join(ROOT, "tests", "golden", "reference_setup_names.json")
REPLACED = {"CKGProtocol": {"GenShare", "AggregateShares"},
            "RKGProtocol": {"GenShareRoundOne", "GenShareRoundTwo", "GenShareRoundThree", "AggregateShareRoundOne", "AggregateShareRoundTwo",
                            "AggregateShareRoundThree", "GenRelinearizationKey"},
            "RKGProtocolNaive": {"GenShareRoundOne", "GenShareRoundTwo", "AggregateShareRoundOne", "AggregateShareRoundTwo", "GenRelinearizationKey"},
            "RTGProtocol": {"genShare", "Aggregate", "Finalize"}}
HELPERS = {"dev", "ReleaseDevice"}
CALLS = {"CKGProtocol": {"CkgShare", "Aggregate"},
         "RKGProtocol": {"RkgRound1", "RkgRound2", "RkgRound3", "RkgKey", "Aggregate", "NewImage", "ShareImage", "PairImage", "DownloadShare", "DownloadPairs"},
         "RKGProtocolNaive": {"RkgNaiveRound1", "RkgNaiveRound2", "RkgNaiveKey", "Aggregate", "NewImage", "PairImage", "DownloadPairs"},
         "RTGProtocol": {"RtgShare", "RtgKey", "Aggregate", "NewImage", "ShareImage", "DownloadShare", "DownloadPairs"}}
RECV = {"CKGProtocol": "ckg", "RKGProtocol": "ekg", "RKGProtocolNaive": "rkg", "RTGProtocol": "rtg"}


def test_delimiters_balance_and_packages():
    for path, package in [(SHIM, "ring")] + [(p, k[0]) for k, p in OVERLAYS.items()]:
        t = _strip(open(path).read())
        for a, b in ("{}", "()", "[]"):
            assert t.count(a) == t.count(b), (path, a, t.count(a), t.count(b))
        assert t.lstrip().startswith("package " + package), path
    for (pkg, proto), path in OVERLAYS.items():
        text = open(path).read()
        assert '"github.com/ldsec/lattigo/ring"' in text, path
        assert ('"github.com/ldsec/lattigo/%s"' % pkg[1:] in text) == (proto != "CKGProtocol"), path      # imported where a signature names it


def test_every_c_call_matches_the_header_and_the_setup_abi_is_reached():
    arity = _header_arity()
    t = _strip(open(SHIM).read())
    seen = set()
    for m in re.finditer(r"\bC\.(lr_[a-z0-9_]+)\s*\(", t):
        sym = m.group(1)
        assert sym in arity, (sym, "not declared in include/lattigo_ring.h")
        assert len(_call_args(t, m.end())) == arity[sym], (sym, arity[sym])
        seen.add(sym)
    abi = {s for s in arity if s.startswith("lr_setup_")}
    assert len(abi) == 21 and abi <= seen, sorted(abi - seen)
    assert seen - abi == {"lr_poly_alloc", "lr_poly_free", "lr_poly_download_limb"}
    # every share call hands over the count of its shares and their handles; the fold the count of its terms
    for m in re.finditer(r"\bC\.lr_setup_(rkg_round[123]|rkg_naive_round[12]|rtg_share)(_device)?\s*\(", t):
        args = [a.strip() for a in _call_args(t, m.end())]
        assert "C.int(len(shares))" in args and args[-1] == "keyHandles(shares)", args
    args = [a.strip() for a in _call_args(t, re.search(r"\bC\.lr_setup_aggregate\s*\(", t).end())]
    assert args[2] == "C.int(n)" and "n := len(shares)" in t
    # the naive rounds pass their bytes in the header's order: round one noise first, round two the planes first
    a1 = [a.strip() for a in _call_args(t, re.search(r"\bC\.lr_setup_rkg_naive_round1\s*\(", t).end())]
    a2 = [a.strip() for a in _call_args(t, re.search(r"\bC\.lr_setup_rkg_naive_round2\s*\(", t).end())]
    assert a1[1] == "C.int(scheme)" and a1[5:8] == ["bytePtr(noise)", "bytePtr(uCoeffs)", "bytePtr(uSigns)"]
    assert a2[5:8] == ["bytePtr(vCoeffs)", "bytePtr(vSigns)", "bytePtr(noise)"]
    header = open(os.path.join(ROOT, "include", "lattigo_ring.h")).read()
    assert "LR_SETUP_BFV = 0, LR_SETUP_CKKS = 1" in header and re.search(r"SetupBFV\s*=\s*0\s*SetupCKKS\s*=\s*1", t)


def test_go_1_13_language_level():
    for path in [SHIM] + list(OVERLAYS.values()):
        t = _strip(open(path).read())
        assert "runtime.Pinner" not in t and "unsafe.Slice" not in t and "unsafe.String" not in t, path
        assert not re.search(r"func \w+\[", t), (path, "type parameters")
        assert not re.search(r"\bany\b", t), path


def test_the_shim_reuses_the_exported_samplers_and_helpers():
    """one set of decision recorders for every handle: the shim defines none of its own and takes bytePtr, keyHandles and polyArray from
    its package"""
    t, samplers = _strip(open(SHIM).read()), _strip(open(SAMPLERS).read())
    for name in ("SampleCompact", "SampleGaussianCompact", "SampleTernaryBits", "bytePtr"):
        assert not re.search(r"func (\([^)]*\) )?%s\(" % name, t), name
        assert re.search(r"func (\([^)]*\) )?%s\(" % name, samplers), name
    assert "crypto/rand" not in open(SHIM).read()
    assert "func polyArray(" in open(os.path.join(ROOT, "go", "ring", "pipelines.go")).read() and "func polyArray(" not in t
    assert "func keyHandles(" in open(os.path.join(ROOT, "go", "ring", "keygen.go")).read() and "func keyHandles(" not in t


def test_overlays_call_what_the_shim_exports():
    shim = open(SHIM).read()
    st = _methods(shim, "Setup")
    assert {"CkgShare": 4, "RkgRound1": 5, "RkgRound2": 5, "RkgRound3": 5, "RkgKey": 3, "RkgNaiveRound1": 7, "RkgNaiveRound2": 7,
            "RkgNaiveKey": 2, "RtgShare": 5, "RtgKey": 3, "Aggregate": 2, "NewImage": 1, "ShareImage": 1, "PairImage": 1, "DownloadShare": 2,
            "DownloadPairs": 2, "Beta": 0}.items() <= st.items()
    for name in ("CkgShare", "RkgRound1", "RkgRound2", "RkgRound3", "RkgNaiveRound1", "RkgNaiveRound2", "RtgShare"):
        assert st[name + "Device"] == st[name], name
    assert re.search(r"func NewSetup\(contextQ, contextP \*Context, maxBatch int\) \*Setup", shim)
    for (pkg, proto), path in OVERLAYS.items():
        t = _strip(open(path).read())
        calls = list(re.finditer(r"\b(?:d|%s\.dev\(\))\.(\w+)\(" % RECV[proto], t))
        assert {m.group(1) for m in calls} == CALLS[proto], (pkg, proto, sorted({m.group(1) for m in calls}))
        for m in calls:
            assert len(_call_args(t, m.end())) == st[m.group(1)], (pkg, proto, m.group(1))
        assert len(_call_args(t, re.search(r"ring\.NewSetup\(", t).end())) == 3
        assert re.search(r"func \(\w+ \*%s\) dev\(\) \*ring\.Setup" % proto, t)
        assert re.search(r"func \(\w+ \*%s\) ReleaseDevice\(\)" % proto, t) and ".Delete(" in t
        if proto == "CKGProtocol":          # contextQP as a ring without P: CKG treats every row alike
            assert re.search(r"ring\.NewSetup\(ckg\.(context|dckksContext\.contextQP), nil, 1\)", t), pkg
        else:
            assert re.search(r"ring\.NewSetup\(\w+\.\w+\.contextQ, \w+\.\w+\.contextP, 1\)", t), (pkg, proto)


def test_the_samplers_are_called_in_upstreams_order():
    for pkg in ("dbfv", "dckks"):
        t = _strip(open(OVERLAYS[(pkg, "RKGProtocolNaive")]).read())
        one = t[t.index(") GenShareRoundOne("):t.index(") AggregateShareRoundOne(")]
        two = t[t.index(") GenShareRoundTwo("):t.index(") AggregateShareRoundTwo(")]
        # round one: the noise of every digit, then the ternaries (relinkey_gen_naive.go:71-107); round two: per digit v, e2, e3 (:139-163)
        assert one.index("i < 2*beta") < one.index("SampleCompact(") < one.index("SampleTernaryBits(")
        assert two.index("SampleTernaryBits(") < two.index("noise[2*i*n") < two.index("noise[(2*i+1)*n")
        assert ("ring.SetupBFV" if pkg == "dbfv" else "ring.SetupCKKS") in one and ("ring.SetupCKKS" if pkg == "dbfv" else "ring.SetupBFV") not in t
        # the three-round protocol and RTG draw beta (round two: 2 beta) noise polys per share, digit after digit
        t = _strip(open(OVERLAYS[(pkg, "RKGProtocol")]).read())
        assert len(re.findall(r"gaussianSampler\.SampleCompact\(noise\[i\*n : \(i\+1\)\*n\]\)", t)) == 3
        assert re.search(r"GenShareRoundTwo\([^{]*\{\s*beta := 2 \* ", t)
        t = _strip(open(OVERLAYS[(pkg, "RTGProtocol")]).read())
        assert len(re.findall(r"gaussianSampler\.SampleCompact\(noise\[i\*n : \(i\+1\)\*n\]\)", t)) == 1
        assert "[]uint64{galEl}" in t and "cannot aggregate shares of different types" in open(OVERLAYS[(pkg, "RTGProtocol")]).read()


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
        # what stays upstream's is named as kept and not defined twice (the marshalers belong to the share types)
        for name in set(up) - REPLACED[proto]:
            assert name in text and not re.search(r"func \(\w+ \*%s\) %s\(" % (proto, name), text), (pkg, proto, name)
        # every field the overlay reads through its receiver or its context exists upstream
        t = _strip(text)
        ctx = "dckksContext" if pkg == "dckks" else "dbfvContext"
        for field in re.findall(r"\b%s\.(\w+)" % RECV[proto], t):
            assert field in ref["fields"][pkg][proto] or field in HELPERS, (pkg, proto, field)
        if not (pkg == "dbfv" and proto == "CKGProtocol"):          # (dbfv's CKGProtocol holds contextQP itself: a ring.Context)
            for field in re.findall(r"\b%s\.(?:dckksContext|context)\.(\w+)" % RECV[proto], t):
                assert field in ref["fields"][pkg][ctx], (pkg, proto, field)
        # the share types the bodies index are upstream's: slices of polys and of pairs
        for name, kind in ref["share_types"][pkg].items():
            if name in text and kind.startswith("["):
                image = "PairImage" if kind.startswith("[][2]") else "ShareImage"
                assert image in text, (pkg, proto, name)
