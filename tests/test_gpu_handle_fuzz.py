"""Seeded differential fuzz of the eight device handles -- lr_bfv_encoder, lr_ckks_encoder, lr_bfv_encryptor / lr_bfv_decryptor,
lr_ckks_encryptor, lr_keygen, lr_collective, lr_refresh, lr_setup -- against their restatements over the CPU oracle (tests/*_ref.py), bit
for bit, on the shapes tests/handle_fuzz_shapes.py draws: degrees 2^1 (2^3 where a handle reads bit planes) .. 2^13 and two seeds at 2^14
and 2^15, 1 .. 8 limbs of Q and 0 .. 4 of P out of the mixed-size modulus pools (61-bit primes, primes next to 2^32, FP64-class and
integer-class limbs in one context), |Q| not a multiple of |P| and |Q| < |P| (the digit loops' break), random levels, batches below
max_batch, keys shared or one per member, host and device-pointer randomness, the three option sets given on the contexts only or on the
handle as well.  Every entry point the shape admits is called.  Outputs are pre-filled with a pattern: limbs above the level keep it, and
so do the members of a larger poly around an output that is wrapped inside it; every input is compared unchanged afterwards.  No case is
skipped: a refusal fails the test unless the header documents it for the shape (a handle without ctxP), and then its code is asserted.
The bodies take (pkg, oracle, seed), so that tools/dbg/long_fuzz.py can run them on seeds beyond the committed ones."""
import ctypes as C

import numpy as np
import pytest

import handle_fuzz_shapes as shapes

pytestmark = pytest.mark.gpu
SEEDS = range(shapes.SEEDS)
ARG = 4                                                                  # LR_ERR_ARG


def _pattern(batch, limbs, N):
    return (np.arange(batch * limbs * N, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 30)).reshape(batch, limbs, N)


def _get(p):
    return p.get().reshape(p.batch, -1, p.N)


class _Case:
    """the contexts of one drawn shape, its output polys (fresh or wrapped inside a larger poly) and the inputs to compare afterwards"""

    def __init__(self, pkg, d):
        self.pkg, self.ring, self.d = pkg, pkg.ring, d
        ring, N = pkg.ring, 1 << d["logn"]
        self.N = N
        self.opt = ring.Options(**shapes.OPTION_SETS[d["options"]])
        self.cQ = ring.NewContextWithParams(N, d["Q"], options=self.opt)
        self.cP = ring.NewContextWithParams(N, d["P"], options=self.opt) if d["P"] else None
        self.handle_opt = self.opt if d["options_on"] == "both" else None    # None: the handle inherits the options of ctxQ
        self.where = (d["family"], d["seed"], d["logn"], len(d["Q"]), len(d["P"]), d["batch"], d["options"], d["options_on"], d["form"])
        self._n_out, self._around, self._inputs = 0, [], []

    def poly(self, x):
        """an input on the device, [batch, limbs, N] or [limbs, N]; compared unchanged by unchanged()"""
        x = np.ascontiguousarray(x, dtype=np.uint64)
        if x.ndim == 2:
            x = x[None]
        p = self.ring.Poly(self.cQ, x.shape[1], x.shape[0]).set(x)
        self._inputs.append((p, x))
        return p

    def out(self, limbs, batch):
        """the next output: a fresh poly holding the pattern, or -- as the shape draws it -- members k .. k + batch - 1 of a larger poly"""
        k = self.d["out"][self._n_out % len(self.d["out"])]
        self._n_out += 1
        if k is None:
            return self.ring.Poly(self.cQ, limbs, batch).set(_pattern(batch, limbs, self.N))
        after = max(1, self.d["max_batch"] - self.d["batch"])               # room for what a pass over max_batch members would write
        pat = _pattern(batch + k + after, limbs, self.N) ^ np.uint64(k)
        big = self.ring.Poly(self.cQ, limbs, batch + k + after).set(pat)
        self._around.append((big, pat, k, batch))
        return self.ring.Poly.wrap(self.cQ, big.device_ptr + 8 * limbs * self.N * k, limbs, batch)

    def pattern_of(self, p):
        """what out() filled p with"""
        for big, pat, k, batch in self._around:
            if p.device_ptr == big.device_ptr + 8 * p.limbs * self.N * k and batch == p.batch and big.limbs == p.limbs:
                return pat[k:k + batch]
        return _pattern(p.batch, p.limbs, self.N)

    def bytes_on_device(self, arrays):
        """arrays one behind the other in device memory, each from a 16-byte boundary (a one-limb poly used as a plain buffer)"""
        N, chunks = self.N, []
        for a in arrays:
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            chunks.append(np.concatenate([raw, np.zeros(-raw.size % 16, dtype=np.uint8)]))
        flat = np.concatenate(chunks)
        words = -(-flat.size // (8 * N)) * N
        buf = np.zeros(words * 8, dtype=np.uint8)
        buf[:flat.size] = flat
        image = buf.view(np.uint64).reshape(words // N, 1, N)
        poly = self.ring.Poly(self.cQ, 1, words // N).set(image)
        self._inputs.append((poly, image))                               # the randomness in device memory is an input too
        ptrs, off = [], 0
        for ch in chunks:
            ptrs.append(poly.device_ptr + off)
            off += ch.size
        return poly, ptrs

    def device_buffer(self, nbytes):
        words = -(-nbytes // (8 * self.N)) * self.N
        return self.ring.Poly(self.cQ, 1, words // self.N).set(np.zeros((words // self.N, 1, self.N), dtype=np.uint64))

    def unchanged(self):
        for big, pat, k, batch in self._around:
            got = _get(big)
            assert np.array_equal(got[:k], pat[:k]) and np.array_equal(got[k + batch:], pat[k + batch:]), self.where + ("words around a wrapped output",)
        for i, (p, x) in enumerate(self._inputs):
            assert np.array_equal(_get(p), x), self.where + ("input %d changed" % i,)

    def refused(self, call, *args, **kw):
        """the refusal the header documents for a handle without ctxP: LR_ERR_ARG"""
        assert self.d["expect_refusal"], self.where
        try:
            call(*args, **kw)
        except self.pkg._native.LatticeRingError as e:
            if e.code != ARG:
                raise                                                    # another error, a HIP error among them, is no mismatch: it ends a long run
        else:
            raise AssertionError(self.where + (self.d["expect_refusal"], "was not refused"))


def _rows_equal(case, got, want, level, pat, what):
    """got [batch, limbs, N] against want[b] = [level + 1, N] per member; limbs above the level keep the pattern"""
    for b in range(got.shape[0]):
        assert np.array_equal(got[b, :level + 1], np.asarray(want[b])[:level + 1]), case.where + (what, b)
    assert np.array_equal(got[:, level + 1:], pat[:, level + 1:]), case.where + (what, "limbs above the level were written")


# ---- lr_bfv_encoder ---------------------------------------------------------------------------------------------------------------------
def bfv_encoder_fuzz(pkg, oracle, seed):
    d = shapes.draw("bfv_encoder", seed)
    c, case = shapes.reference(oracle, d), _Case(pkg, d)
    N, nQ, n, nv = c["N"], c["nQ"], c["n"], c["n_values"]
    enc = pkg.ring.BfvEncoder(case.cQ, c["t"], d["max_batch"], case.handle_opt)
    index, delta = enc.tables()
    assert np.array_equal(index, c["ref"].index) and np.array_equal(delta, c["ref"].delta_mont), case.where + ("tables",)
    keep, ptrs = case.bytes_on_device([c["u"], c["i"]])
    outs = {}
    for name, values, signed, ptr in (("uint", c["u"], False, ptrs[0]), ("int", c["i"], True, ptrs[1])):
        host, dev = case.out(nQ, n), case.out(nQ, n)
        (enc.EncodeInt if signed else enc.EncodeUint)(values, host)
        enc.EncodeDevice(ptr, nv, n, signed, dev)
        want = c["want_i" if signed else "want_u"]
        assert np.array_equal(_get(host), want), case.where + ("encode", name, "host")
        assert np.array_equal(_get(dev), want), case.where + ("encode", name, "device")
        outs[name] = host
    pt = case.poly(c["pt"])
    assert np.array_equal(enc.DecodeUint(pt), c["dec_u"]), case.where + ("decode uint",)
    assert np.array_equal(enc.DecodeInt(pt), c["dec_i"]), case.where + ("decode int",)
    for signed, want in ((False, c["dec_u"]), (True, c["dec_i"])):
        buf = case.device_buffer(8 * n * N)
        enc.DecodeDevice(pt, signed, buf.device_ptr)
        got = buf.get().reshape(-1)[:n * N].reshape(n, N)
        assert np.array_equal(got.view(np.int64) if signed else got, want), case.where + ("decode on the device", signed)
    # what was encoded decodes as the restatement decodes it: where Q leaves room, to the values' residues slot for slot
    back = enc.DecodeUint(outs["uint"])
    assert np.array_equal(back, c["dec_back"]), case.where + ("decode of the encoded plaintext",)
    if c["round_trip_exact"]:
        assert np.array_equal(back[:, :nv], c["u"] % np.uint64(c["t"])) and not back[:, nv:].any(), case.where + ("round trip",)
    case.unchanged()
    del keep


@pytest.mark.parametrize("seed", SEEDS)
def test_bfv_encoder_fuzz(gpu_pkg, oracle, seed):
    bfv_encoder_fuzz(gpu_pkg, oracle, seed)


# ---- lr_ckks_encoder --------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def ckks_encoder_fuzz(pkg, oracle, seed):
    d = shapes.draw("ckks_encoder", seed)
    c, case = shapes.reference(oracle, d), _Case(pkg, d)
    N, nQ, n, slots, level, scale = c["N"], c["nQ"], c["n"], c["slots"], c["level"], c["scale"]
    enc = pkg.ring.CkksEncoder(case.cQ, d["max_batch"], c["roots"], case.handle_opt)
    limbs = level + 1 if d["alias"] else nQ                              # a poly of exactly level + 1 limbs, or of all of them
    keep, ptrs = case.bytes_on_device([c["values"]])
    host, dev = case.out(limbs, n), case.out(limbs, n)
    pat_h, pat_d = case.pattern_of(host), case.pattern_of(dev)
    enc.Encode(host, c["values"], level, scale)
    enc.EncodeDevice(dev, ptrs[0], slots, level, scale, n)
    _rows_equal(case, _get(host), c["want_pt"], level, pat_h, "encode")
    _rows_equal(case, _get(dev), c["want_pt"], level, pat_d, "encode on the device")
    got = enc.Decode(host, slots, level, scale)
    pt = case.poly(c["pt"])
    any_ = enc.Decode(pt, slots, level, scale)
    buf = case.device_buffer(16 * n * slots)
    enc.DecodeDevice(pt, slots, level, scale, buf.device_ptr)
    on_dev = buf.get().reshape(-1)[:2 * n * slots].reshape(n, 2 * slots)
    for b in range(n):
        assert np.array_equal(_bits(got[b]), _bits(c["want_dec"][b])), case.where + ("decode", b)
        assert np.array_equal(_bits(any_[b]), _bits(c["want_dec_any"][b])), case.where + ("decode of any poly", b)
        assert np.array_equal(on_dev[b], _bits(c["want_dec_any"][b])), case.where + ("decode on the device", b)
    case.unchanged()
    del keep


@pytest.mark.parametrize("seed", SEEDS)
def test_ckks_encoder_fuzz(gpu_pkg, oracle, seed, monkeypatch):
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    ckks_encoder_fuzz(gpu_pkg, oracle, seed)


# ---- the two encryptors -----------------------------------------------------------------------------------------------------------------
def _encryptor_fuzz(pkg, oracle, seed, family):
    d = shapes.draw(family, seed)
    c, case = shapes.reference(oracle, d), _Case(pkg, d)
    ring, N, nQ, rows, n, kb = pkg.ring, c["N"], c["nQ"], c["rows"], c["n"], c["kb"]
    ckks = family == "ckks_encryptor"
    level = c["level"] if ckks else nQ - 1
    enc = (ring.CkksEncryptor if ckks else ring.BfvEncryptor)(case.cQ, case.cP, d["max_batch"], options=case.handle_opt)
    sk, pk, crp, pt = case.poly(c["sk"]), (case.poly(c["pk0"]), case.poly(c["pk1"])), case.poly(c["crp"]), case.poly(c["pt"])
    # the fast forms read |Q| limbs: keys over Q alone serve them too
    sk_q, pk_q, crp_q = case.poly(c["sk"][:, :nQ]), (case.poly(c["pk0"][:, :nQ]), case.poly(c["pk1"][:, :nQ])), case.poly(c["crp"][:, :nQ])
    rand = [c["uc"], c["us"], c["e0"], c["e1"], c["e"]]
    keep, ptrs = case.bytes_on_device(rand)
    lvl = (level,) if ckks else ()
    first = True
    for form, fast in c["forms"]:
        # the drawn form of the randomness for every entry point, the other form once
        for on_device in ((d["form"] == "device",) + ((d["form"] != "device",) if first else ())):
            ct = (case.out(nQ, n), case.out(nQ, n))
            pats = [case.pattern_of(p) for p in ct]
            over_q = fast and d["alias"]
            if form == "pk":
                keys = pk_q if over_q else pk
                if on_device:
                    enc.EncryptPkDevice(keys, ptrs[0:2], ptrs[2:4], pt, ct, *lvl, fast=fast)
                else:
                    enc.EncryptPk(keys, rand[0:2], rand[2:4], pt, ct, *lvl, fast=fast)
            else:
                key, a = (sk_q, crp_q) if over_q else (sk, crp)
                if on_device:
                    enc.EncryptSkDevice(key, a, ptrs[4], pt, ct, *lvl, fast=fast)
                else:
                    enc.EncryptSk(key, a, rand[4], pt, ct, *lvl, fast=fast)
            for k in range(2):
                _rows_equal(case, _get(ct[k]), [w[k] for w in c["want"][(form, fast)]], level, pats[k], (form, fast, on_device, k))
        first = False
    if not c["nP"]:
        ct = (case.out(nQ, n), case.out(nQ, n))
        case.refused(enc.EncryptPk, pk_q, rand[0:2], rand[2:4], pt, ct, *lvl, fast=False)
        case.refused(enc.EncryptSk, sk_q, crp_q, rand[4], pt, ct, *lvl, fast=False)
    if not ckks:
        dec = ring.BfvDecryptor(case.cQ, d["max_batch"])
        comps = [case.poly(x) for x in c["ct"]]
        out = dec.Decrypt(comps, sk_q if d["alias"] else sk, case.out(nQ, n))       # the first |Q| limbs of the key are read
        got = _get(out)
        for b in range(n):
            assert np.array_equal(got[b], c["want_dec"][b]), case.where + ("decrypt", c["degree"], b)
        if d["alias"]:                                                   # pt_out may be ct[degree]
            top = ring.Poly(case.cQ, nQ, n).set(c["ct"][-1])
            dec.Decrypt(comps[:-1] + [top], sk, top)
            assert np.array_equal(_get(top), got), case.where + ("decrypt in place",)
    case.unchanged()
    del keep


def bfv_encryptor_fuzz(pkg, oracle, seed):
    _encryptor_fuzz(pkg, oracle, seed, "bfv_encryptor")


def ckks_encryptor_fuzz(pkg, oracle, seed):
    _encryptor_fuzz(pkg, oracle, seed, "ckks_encryptor")


@pytest.mark.parametrize("seed", SEEDS)
def test_bfv_encryptor_fuzz(gpu_pkg, oracle, seed):
    bfv_encryptor_fuzz(gpu_pkg, oracle, seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_ckks_encryptor_fuzz(gpu_pkg, oracle, seed):
    ckks_encryptor_fuzz(gpu_pkg, oracle, seed)


# ---- lr_keygen --------------------------------------------------------------------------------------------------------------------------
def _key_images(case, c, a):
    """one key image per entry of a: the pattern in the even members, the caller's uniform polys in the odd ones"""
    keys, pats = [], []
    for k in range(len(a)):
        key = case.out(c["rows"], 2 * c["beta"])
        img = case.pattern_of(key).copy()
        img[1::2] = a[k]
        keys.append(key.set(img))
        pats.append(img)
    return keys, pats


def _check_keys(case, keys, wants, a, what):
    for k, (key, want) in enumerate(zip(keys, wants)):
        got = _get(key)
        assert np.array_equal(got[0::2], want[0::2]), case.where + (what, k, "evakey[i][0]")
        assert np.array_equal(got[1::2], a[k]), case.where + (what, k, "the uniform half changed")


def keygen_fuzz(pkg, oracle, seed):
    d = shapes.draw("keygen", seed)
    c, case = shapes.reference(oracle, d), _Case(pkg, d)
    ring, N, rows, n = pkg.ring, c["N"], c["rows"], c["n"]
    kg = ring.KeyGenerator(case.cQ, case.cP, d["max_batch"], options=case.handle_opt)
    rand = [c["uc"], c["us"], c["pk_e"]] + ([c["e"]] if c["nP"] else [])
    keep, ptrs = case.bytes_on_device(rand)
    on_device = d["form"] == "device"
    sk = case.out(rows, n)
    kg.GenSecretKeyDevice(ptrs[0:2], sk) if on_device else kg.GenSecretKey(rand[0:2], sk)
    assert np.array_equal(_get(sk), c["sk"]), case.where + ("sk",)
    other = case.out(rows, n)                                            # the other form of the randomness, once
    kg.GenSecretKey(rand[0:2], other) if on_device else kg.GenSecretKeyDevice(ptrs[0:2], other)
    assert np.array_equal(_get(other), c["sk"]), case.where + ("sk, the other form",)
    sk_in, pk = case.poly(c["sk"][:c["kb"]]), (case.out(rows, n), case.poly(c["pk1"]))
    kg.GenPublicKeyDevice(sk_in, ptrs[2], pk) if on_device else kg.GenPublicKey(sk_in, rand[2], pk)
    assert np.array_equal(_get(pk[0]), c["pk0"]), case.where + ("pk0",)
    if not c["nP"]:
        case.refused(kg.NewSwitchingKey)
        case.refused(lambda: pkg._native.check(pkg._native.lib().lr_keygen_relin_keys(
            kg.h, sk_in.h, 1, c["pk_e"].ctypes.data_as(C.c_void_p), (C.c_void_p * 1)(sk.h.value))))
        case.unchanged()
        return
    e, a = (ptrs[3] if on_device else rand[3]), c["a"]
    dev = "Device" if on_device else ""
    sk_out, sk0 = case.poly(c["sk_out"]), case.poly(c["sk"][:1])
    keys, _ = _key_images(case, c, a)
    getattr(kg, "GenSwitchingKeys" + dev)(sk_in, sk_out, e, keys)
    _check_keys(case, keys, c["swk"], a, "swk")
    keys, _ = _key_images(case, c, a)
    getattr(kg, "GenRelinKeys" + dev)(sk0, e, keys)
    _check_keys(case, keys, c["rlk"], a, "rlk")
    keys, _ = _key_images(case, c, a)
    getattr(kg, "GenRotationKeys" + dev)(sk0, c["gens"], e, keys)
    _check_keys(case, keys, c["rot"], a, ("rot", tuple(c["gens"])))
    case.unchanged()
    del keep


@pytest.mark.parametrize("seed", SEEDS)
def test_keygen_fuzz(gpu_pkg, oracle, seed):
    keygen_fuzz(gpu_pkg, oracle, seed)


# ---- lr_collective ----------------------------------------------------------------------------------------------------------------------
def _fold(case, handle, shares, want, level, base=None, alias=False):
    """a fold of `shares` ([batch, limbs, N] each) into a fresh output, and -- with alias -- into shares[0] and into the base"""
    n, limbs = shares[0].shape[0], shares[0].shape[1]
    dev = [case.poly(s) for s in shares]
    dbase = case.poly(base) if base is not None else None
    out = case.out(limbs, n)
    pat = case.pattern_of(out)
    handle.Aggregate(dev, out, level, **({"base": dbase} if base is not None else {}))
    got = _get(out)
    assert np.array_equal(got[:, :level + 1], want), case.where + ("fold", len(shares), base is not None)
    assert np.array_equal(got[:, level + 1:], pat[:, level + 1:]), case.where + ("fold", "limbs above the level were written")
    if alias:
        for target in ["share0"] + (["base"] if base is not None else []):
            mine = [case.ring.Poly(case.cQ, limbs, n).set(s) for s in shares]
            mbase = case.ring.Poly(case.cQ, limbs, n).set(base) if base is not None else None
            o = mine[0] if target == "share0" else mbase
            before = _get(o)
            handle.Aggregate(mine, o, level, **({"base": mbase} if base is not None else {}))
            assert np.array_equal(_get(o)[:, :level + 1], want), case.where + ("fold into", target)
            assert np.array_equal(_get(o)[:, level + 1:], before[:, level + 1:]), case.where + ("fold into", target, "limbs above the level")


def collective_fuzz(pkg, oracle, seed):
    d = shapes.draw("collective", seed)
    c, case = shapes.reference(oracle, d), _Case(pkg, d)
    nQ, n, level = c["nQ"], c["n"], c["level"]
    col = pkg.ring.Collective(case.cQ, case.cP, d["max_batch"], options=case.handle_opt)
    over_q = d["alias"]                                                  # |Q| limbs suffice for the secret keys
    sk_in, sk_out = case.poly(c["sk_in"][:, :nQ] if over_q else c["sk_in"]), case.poly(c["sk_out"][:, :nQ] if over_q else c["sk_out"])
    pk, c1 = (case.poly(c["pk0"]), case.poly(c["pk1"])), case.poly(c["c1"])
    rand = [c["e"][0], c["uc"], c["us"], c["e"][1], c["e"][2]]
    keep, ptrs = case.bytes_on_device(rand)
    for on_device in (d["form"] == "device", d["form"] != "device"):
        r = ptrs if on_device else rand
        dev = "Device" if on_device else ""
        for scheme, lvl, args in (("ckks", level, (level,)), ("bfv", nQ - 1, ())):
            share, o0, o1 = case.out(nQ, n), case.out(nQ, n), case.out(nQ, n)
            pats = [case.pattern_of(p) for p in (share, o0, o1)]
            name = "Ckks" if scheme == "ckks" else "Bfv"
            getattr(col, name + "CksShare" + dev)(sk_in, sk_out, c1, r[0], share, *args)
            getattr(col, name + "PcksShare" + dev)(sk_in, pk, c1, r[1:3], r[3:5], (o0, o1), *args)
            _rows_equal(case, _get(share), c[scheme + "_cks"], lvl, pats[0], (scheme, "cks", on_device))
            _rows_equal(case, _get(o0), [w[0] for w in c[scheme + "_pcks"]], lvl, pats[1], (scheme, "pcks out0", on_device))
            _rows_equal(case, _get(o1), [w[1] for w in c[scheme + "_pcks"]], lvl, pats[2], (scheme, "pcks out1", on_device))
    _fold(case, col, c["shares"], c["fold"], level, alias=d["alias"])
    _fold(case, col, c["shares"], c["fold_base"], level, base=c["base"], alias=d["alias"])
    case.unchanged()
    del keep


@pytest.mark.parametrize("seed", SEEDS)
def test_collective_fuzz(gpu_pkg, oracle, seed):
    collective_fuzz(gpu_pkg, oracle, seed)


# ---- lr_refresh -------------------------------------------------------------------------------------------------------------------------
def refresh_fuzz(pkg, oracle, seed):
    d = shapes.draw("refresh", seed)
    c, case = shapes.reference(oracle, d), _Case(pkg, d)
    ring, N, nQ, n, ls = pkg.ring, c["N"], c["nQ"], c["n"], c["level_start"]
    r = ring.Refresh(case.cQ, case.cP, c["t"] if c["bfv"] else 0, d["max_batch"], options=case.handle_opt)
    assert r.MaskWords(ls) == c["words"], case.where + ("mask words",)
    sk_qp, sk_q = case.poly(c["sk"]), case.poly(c["sk"][:, :nQ])
    c1, crs, dec_in, rec_in = case.poly(c["c1"]), case.poly(c["crs"]), case.poly(c["dec"]), case.poly(c["rec"])
    planes = pkg.sampling.mask_word_planes(c["mask"], c["words"])
    rand = [planes, c["e"][0], c["e"][1]] + ([c["mask_bfv"]] if c["bfv"] else [])
    keep, ptrs = case.bytes_on_device(rand)
    for on_device in (d["form"] == "device", d["form"] != "device"):
        dec, rec = case.out(nQ, n), case.out(nQ, n)
        pat = case.pattern_of(dec)
        sk = sk_qp if on_device else sk_q                                # |Q| limbs suffice for the CKKS calls
        if on_device:
            r.CkksGenSharesDevice(sk, ls, c1, crs, ptrs[0], ptrs[1:3], (dec, rec))
        else:
            r.CkksGenShares(sk, ls, c1, crs, planes, rand[1:3], (dec, rec))
        _rows_equal(case, _get(dec), [w[0] for w in c["ckks_shares"]], ls, pat, ("share_decrypt", on_device))
        gr = _get(rec)
        for b in range(n):
            assert np.array_equal(gr[b], c["ckks_shares"][b][1]), case.where + ("share_recrypt", on_device, b)
    summed, c0_at = case.poly(c["sum"]), case.poly(c["c0_at"])
    go, gf = _get(r.CkksRecode(ls, summed, case.out(nQ, n))), _get(r.CkksFinalize(ls, c0_at, (dec_in, rec_in), case.out(nQ, n)))
    for b in range(n):
        assert np.array_equal(go[b], c["recode"][b]), case.where + ("recode", b)
        assert np.array_equal(gf[b], c["ckks_finalize"][b]), case.where + ("finalize", b)
    if d["alias"]:                                                       # out may be in, out0 may be c0: polys of all of Q then
        full = np.stack([np.concatenate([x, _pattern(1, nQ - ls - 1, N)[0]]) for x in c["sum"]]) if ls < nQ - 1 else c["sum"]
        p = ring.Poly(case.cQ, nQ, n).set(full)
        assert np.array_equal(_get(r.CkksRecode(ls, p, p)), go), case.where + ("recode in place",)
        full = np.stack([np.concatenate([x, _pattern(1, nQ - ls - 1, N)[0]]) for x in c["c0_at"]]) if ls < nQ - 1 else c["c0_at"]
        p = ring.Poly(case.cQ, nQ, n).set(full)
        assert np.array_equal(_get(r.CkksFinalize(ls, p, (dec_in, rec_in), p)), gf), case.where + ("finalize in place",)
    if c["bfv"]:
        crs_qp, c0 = case.poly(c["crs_qp"]), case.poly(c["c0"])
        for on_device in (d["form"] == "device", d["form"] != "device"):
            dec, rec = case.out(nQ, n), case.out(nQ, n)
            if on_device:
                r.BfvGenSharesDevice(sk_qp, c1, crs_qp, ptrs[3], ptrs[1:3], (dec, rec))
            else:
                r.BfvGenShares(sk_qp, c1, crs_qp, rand[3], rand[1:3], (dec, rec))
            gd, gr = _get(dec), _get(rec)
            for b in range(n):
                assert np.array_equal(gd[b], c["bfv_shares"][b][0]), case.where + ("bfv share_decrypt", on_device, b)
                assert np.array_equal(gr[b], c["bfv_shares"][b][1]), case.where + ("bfv share_recrypt", on_device, b)
        out = r.BfvFinalize(c0, crs_qp, (dec_in, rec_in), (case.out(nQ, n), case.out(nQ, n)))
        g0, g1 = _get(out[0]), _get(out[1])
        for b in range(n):
            assert np.array_equal(g0[b], c["bfv_finalize"][b][0]) and np.array_equal(g1[b], c["bfv_finalize"][b][1]), case.where + ("bfv finalize", b)
        if d["alias"]:
            p = ring.Poly(case.cQ, nQ, n).set(c["c0"])
            assert np.array_equal(_get(r.BfvFinalize(p, crs_qp, (dec_in, rec_in), (p, case.out(nQ, n)))[0]), g0), case.where + ("bfv finalize, out0 = c0",)
    else:
        case.refused(r.BfvGenShares, sk_q, c1, crs, np.zeros((n, N), dtype=np.uint64), rand[1:3], (case.out(nQ, n), case.out(nQ, n)))
        case.refused(r.BfvFinalize, c1, crs, (dec_in, rec_in), (case.out(nQ, n), case.out(nQ, n)))
    _fold(case, r, c["shares"], c["fold"], c["level"], alias=d["alias"])
    case.unchanged()
    del keep


@pytest.mark.parametrize("seed", SEEDS)
def test_refresh_fuzz(gpu_pkg, oracle, seed):
    refresh_fuzz(gpu_pkg, oracle, seed)


# ---- lr_setup ---------------------------------------------------------------------------------------------------------------------------
def setup_fuzz(pkg, oracle, seed):
    d = shapes.draw("setup", seed)
    c, case = shapes.reference(oracle, d), _Case(pkg, d)
    ring, N, rows, n, beta, w = pkg.ring, c["N"], c["rows"], c["n"], c["beta"], c["want"]
    st = ring.Setup(case.cQ, case.cP, d["max_batch"], options=case.handle_opt)
    assert st.rows == rows
    on_device = d["form"] == "device"
    dev = "Device" if on_device else ""
    names = ["ckg_e"] + (["r1_e", "r2_e", "r3_e", "n1_e", "n2_e", "rtg_e"] if c["nP"] else [])
    rand = {k: c[k] for k in names}
    if c["nP"]:
        rand.update(n1c=c["n1_bits"][0], n1s=c["n1_bits"][1], n2c=c["n2_bits"][0], n2s=c["n2_bits"][1])
    keep, ptr_list = case.bytes_on_device(list(rand.values()))
    ptr = dict(zip(rand, ptr_list))
    r = (lambda k: ptr[k]) if on_device else (lambda k: rand[k])
    call = lambda fn, *args: getattr(st, fn + dev)(*args)
    sk, u, crs = case.poly(c["sk"]), case.poly(c["u"]), case.poly(c["crs"])

    def check(shares, kind):
        for k, s in enumerate(shares):
            assert np.array_equal(_get(s), w[kind][k]), case.where + (kind, k)
    share = case.out(rows, n)
    call("CkgShare", sk, crs, r("ckg_e"), share)
    got = _get(share)
    for k in range(n):
        assert np.array_equal(got[k], w["ckg"][k]), case.where + ("ckg", k)
    other = case.out(rows, n)                                            # the other form of the randomness, once
    (st.CkgShare if on_device else st.CkgShareDevice)(sk, crs, rand["ckg_e"] if on_device else ptr["ckg_e"], other)
    assert np.array_equal(_get(other), got), case.where + ("ckg, the other form",)
    members = c["shares"][0].shape[0]
    polys = [case.poly(s) for s in c["shares"]]
    out = st.Aggregate(polys, case.out(rows, members))
    assert np.array_equal(_get(out).reshape(w["fold"].shape), w["fold"]), case.where + ("fold", members, len(polys))
    if d["alias"]:
        mine = [ring.Poly(case.cQ, rows, members).set(s) for s in c["shares"]]
        st.Aggregate(mine, mine[-1])
        assert np.array_equal(_get(mine[-1]).reshape(w["fold"].shape), w["fold"]), case.where + ("fold in place",)
    if not c["nP"]:
        case.refused(st.NewShare)
        one = ring.Poly(case.cQ, rows, 1)
        case.refused(lambda: pkg._native.check(pkg._native.lib().lr_setup_rtg_key(st.h, one.h, one.h, share.h)))
        case.unchanged()
        return
    new = lambda m: [case.out(rows, m) for _ in range(n)]
    crp, sk0 = case.poly(c["crp"]), case.poly(c["sk"][:1])
    inp = {k: case.poly(c[k]) for k in ("pk0", "r1_sum", "r2_sum", "r3_sum", "n1_sum", "n2_sum")}
    pk = (inp["pk0"], crs)
    check(call("RkgRound1", u, sk, crp, r("r1_e"), new(beta)), "r1")
    check(call("RkgRound2", inp["r1_sum"], sk, crp, r("r2_e"), new(2 * beta)), "r2")
    check(call("RkgRound3", inp["r2_sum"], u, sk, r("r3_e"), new(beta)), "r3")
    bits1, bits2 = (r("n1c"), r("n1s")), (r("n2c"), r("n2s"))
    check(call("RkgNaiveRound1", st.BFV, sk, pk, r("n1_e"), bits1, new(2 * beta)), "n1_bfv")
    check(call("RkgNaiveRound1", st.CKKS, sk, pk, r("n1_e"), bits1, new(2 * beta)), "n1_ckks")
    check(call("RkgNaiveRound2", inp["n1_sum"], sk, pk, bits2, r("n2_e"), new(2 * beta)), "n2")
    check(call("RtgShare", sk0, c["gens"], crp, r("rtg_e"), new(beta)), "rtg")
    # the finalize steps have no randomness
    assert np.array_equal(_get(st.RkgKey(inp["r2_sum"], inp["r3_sum"], case.out(rows, 2 * beta))), w["rlk"]), case.where + ("rlk",)
    assert np.array_equal(_get(st.RkgNaiveKey(inp["n2_sum"], case.out(rows, 2 * beta))), w["rlk_naive"]), case.where + ("naive rlk",)
    assert np.array_equal(_get(st.RtgKey(inp["r1_sum"], crp, case.out(rows, 2 * beta))), w["rot"]), case.where + ("rot",)
    if d["alias"]:                                                       # in place: evk_out == round2
        r2 = ring.Poly(case.cQ, rows, 2 * beta).set(c["r2_sum"])
        assert np.array_equal(_get(st.RkgKey(r2, inp["r3_sum"], r2)), w["rlk"]), case.where + ("rlk in place",)
        r2 = ring.Poly(case.cQ, rows, 2 * beta).set(c["n2_sum"])
        assert np.array_equal(_get(st.RkgNaiveKey(r2, r2)), w["rlk_naive"]), case.where + ("naive rlk in place",)
    case.unchanged()
    del keep


@pytest.mark.parametrize("seed", SEEDS)
def test_setup_fuzz(gpu_pkg, oracle, seed):
    setup_fuzz(gpu_pkg, oracle, seed)


BODIES = {"bfv_encoder": bfv_encoder_fuzz, "ckks_encoder": ckks_encoder_fuzz, "bfv_encryptor": bfv_encryptor_fuzz,
          "ckks_encryptor": ckks_encryptor_fuzz, "keygen": keygen_fuzz, "collective": collective_fuzz, "refresh": refresh_fuzz,
          "setup": setup_fuzz}
