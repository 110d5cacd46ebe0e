"""The key generator's Go side cannot be compiled here (no Go toolchain in the image): go/ring/keygen.go (the cgo type KeyGenerator; the compact
samplers are those of go/ring/bfv_encryptor.go) and go/ckks/keygen_device.go, go/bfv/keygen_device.go (replacement bodies for GenPublicKey,
GenRelinKey, GenSwitchingKey, GenRot, GenRotationKeysPow2, newSwitchingKey and genrotKey) are checked statically, in the manner of
test_go_ckks_encryptor.py -- every C symbol called is declared in include/lattigo_ring.h with the same number of arguments and every
lr_keygen_* symbol of the header is reached, delimiters balance, the go 1.13 language level holds, the overlays call only what the shim
has, with its arity, their methods keep the upstream signatures (tests/golden/reference_keygen_names.json) and the evaluators' keyImage
finds the generated images."""
import json
import os
import re

from conftest import ROOT
from test_go_bfv_encoder import _call_args
from test_go_bfv_encryptor import _methods
from test_go_shim import _header_arity, _split_args, _strip

SHIM = os.path.join(ROOT, "go", "ring", "keygen.go")
SAMPLERS = os.path.join(ROOT, "go", "ring", "bfv_encryptor.go")
OVERLAYS = {"ckks": os.path.join(ROOT, "go", "ckks", "keygen_device.go"), "bfv": os.path.join(ROOT, "go", "bfv", "keygen_device.go")}
EVALUATORS = {"ckks": os.path.join(ROOT, "go", "ckks", "evaluator_device.go"), "bfv": os.path.join(ROOT, "go", "bfv", "evaluator_device.go")}
NAMES = os.path.join(ROOT, "tests", "golden", "reference_keygen_names.json")
REPLACED = {"ckks": {"GenPublicKey", "GenRelinKey", "GenSwitchingKey", "GenRot", "GenRotationKeysPow2", "newSwitchingKey", "genrotKey"},
            "bfv": {"GenPublicKey", "GenRelinKey", "GenSwitchingKey", "GenRot", "GenRotationKeysPow2", "genrotkey"}}
HELPERS = {"dev", "ReleaseDevice", "ReleaseGeneratedKey", "sampleKey", "image", "finish"}


def test_delimiters_balance_and_packages():
    for path, package in [(SHIM, "ring")] + [(p, k) for k, p in OVERLAYS.items()]:
        t = _strip(open(path).read())
        for a, b in ("{}", "()", "[]"):
            assert t.count(a) == t.count(b), (path, a, t.count(a), t.count(b))
        assert t.lstrip().startswith("package " + package), path
    for path in OVERLAYS.values():
        assert '"github.com/ldsec/lattigo/ring"' in open(path).read()


def test_every_c_call_matches_the_header_and_the_keygen_abi_is_reached():
    arity = _header_arity()
    t = _strip(open(SHIM).read())
    seen = set()
    for m in re.finditer(r"\bC\.(lr_[a-z0-9_]+)\s*\(", t):
        sym = m.group(1)
        assert sym in arity, (sym, "not declared in include/lattigo_ring.h")
        assert len(_call_args(t, m.end())) == arity[sym], (sym, arity[sym])
        seen.add(sym)
    abi = {s for s in arity if s.startswith("lr_keygen_")}
    assert len(abi) == 13 and abi <= seen, sorted(abi - seen)
    assert seen - abi == {"lr_poly_alloc", "lr_poly_free", "lr_poly_download_limb"}
    # every switching-key call hands over the count of its images and their handles
    for m in re.finditer(r"\bC\.lr_keygen_(switching|relin|rotation)_keys(_device)?\s*\(", t):
        args = [a.strip() for a in _call_args(t, m.end())]
        assert "C.int(len(images))" in args and args[-1] == "keyHandles(images)", args


def test_go_1_13_language_level():
    for path in [SHIM] + list(OVERLAYS.values()):
        t = _strip(open(path).read())
        assert "runtime.Pinner" not in t and "unsafe.Slice" not in t and "unsafe.String" not in t, path
        assert not re.search(r"func \w+\[", t), (path, "type parameters")
        assert not re.search(r"\bany\b", t), path


def test_the_shim_reuses_the_exported_samplers():
    """one set of decision recorders for every handle: the shim defines none of its own and needs bytePtr from its package"""
    t, samplers = _strip(open(SHIM).read()), _strip(open(SAMPLERS).read())
    for name in ("SampleCompact", "SampleGaussianCompact", "SampleTernaryBits", "bytePtr"):
        assert not re.search(r"func (\([^)]*\) )?%s\(" % name, t), name
        assert re.search(r"func (\([^)]*\) )?%s\(" % name, samplers), name
    assert "crypto/rand" not in open(SHIM).read()


def test_overlays_call_what_the_shim_exports():
    shim = open(SHIM).read()
    kg = _methods(shim, "KeyGenerator")
    assert {"GenSecretKey": 3, "GenPublicKey": 3, "GenSwitchingKeys": 4, "GenRelinKeys": 3, "GenRotationKeys": 4, "NewSwitchingKeyImage": 1,
            "DownloadKey": 2, "Beta": 0}.items() <= kg.items()
    for name in ("GenSecretKey", "GenPublicKey", "GenSwitchingKeys", "GenRelinKeys", "GenRotationKeys"):
        assert kg[name + "Device"] == kg[name], name
    assert re.search(r"func NewKeyGenerator\(contextQ, contextP \*Context, maxBatch int\) \*KeyGenerator", shim)
    for pkg, path in OVERLAYS.items():
        t = _strip(open(path).read())
        calls = list(re.finditer(r"\.dev\(\)\.(\w+)\(", t))
        assert {m.group(1) for m in calls} == {"GenPublicKey", "GenSwitchingKeys", "GenRelinKeys", "GenRotationKeys", "NewSwitchingKeyImage", "DownloadKey"}, pkg
        for m in calls:
            assert len(_call_args(t, m.end())) == kg[m.group(1)], (pkg, m.group(1))
        found = list(re.finditer(r"\bSampleCompact\(", t))
        assert len(found) == 2, pkg                                   # the public key's noise and the per-digit noise of sampleKey
        for m in found:
            assert len(_call_args(t, m.end())) == 1
        assert len(_call_args(t, re.search(r"ring\.NewKeyGenerator\(", t).end())) == 3
        assert re.search(r"func \(\w+ \*keyGenerator\) dev\(\) \*ring\.KeyGenerator", t)
        # per digit upstream's order: the noise, then the uniform poly
        body = t[t.index("sampleKey(noise []byte)"):]
        assert body.index("SampleCompact(e)") < body.index("NewUniformPoly()")
        # GenRotationKeysPow2 makes its whole set in one call
        pow2 = t[t.index("GenRotationKeysPow2("):]
        assert pow2.count(".dev().GenRotationKeys(") == 1 and "for i, k := range keys" in pow2


def test_replacement_bodies_keep_the_upstream_signatures():
    ref = json.load(open(NAMES))
    for pkg, path in OVERLAYS.items():
        up, text = ref["signatures"][pkg], open(path).read()
        mine = {}
        for m in re.finditer(r"func (?:\(\w+ \*keyGenerator\) )?(\w+)\(([^)]*)\)([^{]*)\{", text):
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
            assert name not in up and name not in ref["fields"][pkg]["keyGenerator"], (pkg, name)
        # what stays upstream's is named as kept and not defined twice
        for name in set(up) - REPLACED[pkg] - {"newswitchingkey"}:
            assert name in text and not re.search(r"func \(\w+ \*keyGenerator\) %s\(" % name, text), (pkg, name)
        if pkg == "bfv":
            assert re.search(r"delete\s+newswitchingkey\b", text) and "func (keygen *keyGenerator) newswitchingkey(" not in text
        for ident in ref["upstream_identifiers_found"][pkg]:
            assert ident in text, (pkg, ident)
        # every field the overlay reads through a key or its receiver exists upstream
        t = _strip(text)
        for field in re.findall(r"\bkeygen\.(\w+)", t):
            assert field in ref["fields"][pkg]["keyGenerator"] or field in HELPERS or field in up, (pkg, field)
        for field in re.findall(r"\brotKey\.(\w+)", t):
            assert field in ref["fields"][pkg]["RotationKeys"], (pkg, field)
        for field in re.findall(r"\b(?:k|evk|switchingkey|switchkey)\.(evakey)\b", t):
            assert field in ref["fields"][pkg]["SwitchingKey"]


def test_beta_refuses_a_handle_without_p():
    t = _strip(open(SHIM).read())
    body = t[t.index("func (g *KeyGenerator) Beta() int"):]
    assert body.index("g.contextP == nil") < body.index("len(g.contextP.Modulus)")


def test_the_evaluators_find_generated_images_without_an_upload():
    for pkg in ("ckks", "bfv"):
        ev, kg = _strip(open(EVALUATORS[pkg]).read()), _strip(open(OVERLAYS[pkg]).read())
        assert re.search(r"var generatedKeyImages sync\.Map", kg) and "generatedKeyImages.Store(k, img)" in kg
        body = ev[ev.index("keyImage(k *SwitchingKey)"):]
        assert body.index("generatedKeyImages.Load(k)") < body.index("SwitchingKeyImage(k.evakey)")
        # the global map does not keep an image alive for the life of the process: the evaluator takes it over, and a key no evaluator
        # took has a release path
        assert body.index("generatedKeyImages.Load(k)") < body.index("generatedKeyImages.Delete(k)") < body.index("SwitchingKeyImage(k.evakey)")
        assert re.search(r"func ReleaseGeneratedKey\(k \*SwitchingKey\) \{\s*generatedKeyImages\.Delete\(k\)", kg), pkg
