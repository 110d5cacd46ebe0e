"""ckks.Encoder on the device (lr_ckks_encoder, ring.CkksEncoder) against its line-by-line restatement (tests/ckks_encoder_ref.py), bit for
bit, with the root table of Python's math.cos / math.sin on both sides: Encode and Decode on the fused route (slots <= 2^13) and on the
tiled one (forced through the option field and the environment override, natural at 2^14 and 2^15 slots), for 1, 2 and 6 limbs of Qi60 and
the moduli of PN12QP109, levels below the poly's limb count, batches 1, 3 and max_batch, scales 2^30 / 2^40 / 2^55, coefficients on both
branches of scaleUpVecExact, Decode of random and of boundary plaintexts through the whole multi-word conversion, the device-pointer entry
points, the tables, every refusal, and Encode -> EncryptPk -> Decrypt -> Decode end to end."""
import ctypes as C
import math

import numpy as np
import pytest

import ckks_encoder_ref as ref

pytestmark = pytest.mark.gpu

MAX_BATCH = 4
_roots, _refs = {}, {}


def _Q(pkg, spec):
    """'qi60:k' = the first k primes of Qi60 (1 mod 2^18: every N here); otherwise a CKKS parameter set's Q"""
    if spec.startswith("qi60:"):
        return list(pkg.params.Qi60()[:int(spec[5:])])
    return list(pkg.params.ckks_moduli(spec)[1])


def _root_table(N):
    if N not in _roots:
        _roots[N] = ref.roots_table(N)
    return _roots[N]


def _ref(oracle, pkg, logn, qspec):
    if (logn, qspec) not in _refs:
        _refs[(logn, qspec)] = ref.Encoder(oracle, 1 << logn, _Q(pkg, qspec), _root_table(1 << logn))
    return _refs[(logn, qspec)]


def _values(slots, b, seed=0):
    """slot values of batch element b inside the unit disc; element 1 has zeros and exact halves among them"""
    rng = np.random.default_rng(31 * slots + 7 * b + seed)
    v = rng.uniform(0, 1, slots) * np.exp(2j * math.pi * rng.uniform(0, 1, slots))
    if b == 1:
        v[::3] = 0
        v[1::5] = 0.5 - 0.25j
    return v


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _sentinel(limbs, N, batch):
    return (np.arange(batch * limbs * N, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 30)).reshape(batch, limbs, N)


def _check(oracle, pkg, enc, cQ, logn, qspec, slots, level, scale, batch, vals=None):
    """Encode and Decode of `batch` plaintexts against the restatement; the limbs above `level` keep what they held"""
    N, r = 1 << logn, _ref(oracle, pkg, logn, qspec)
    limbs = len(cQ.Modulus)
    if vals is None:
        vals = np.stack([_values(slots, b) for b in range(batch)])
    mark = _sentinel(limbs, N, batch)
    pt = enc.Encode(cQ.NewPoly(batch).set(mark), vals, level, scale)
    got_pt = pt.get().reshape(batch, limbs, N)
    got = enc.Decode(pt, slots, level, scale)
    assert got.shape == (batch, slots)
    for b in range(batch):
        want_pt = r.encode(vals[b], level, scale)
        assert np.array_equal(got_pt[b, :level + 1], want_pt), (slots, level, b)
        assert np.array_equal(got_pt[b, level + 1:], mark[b, level + 1:]), (slots, level, b)
        assert np.array_equal(_bits(got[b]), _bits(r.decode(want_pt, slots, level, scale))), (slots, level, b)
    return pt, got


def _small(N, bound, seed):
    return np.random.default_rng(seed).integers(-bound, bound + 1, size=N)


def _residues(v, moduli):
    return np.array([[int(x) % q for x in v] for q in moduli], dtype=np.uint64)


def _mont(a, moduli):
    return np.array([[(int(x) << 64) % q for x in a[i]] for i, q in enumerate(moduli)], dtype=np.uint64)


def _encoder(pkg, logn, qspec, max_batch=MAX_BATCH, options=None):
    cQ = pkg.ring.NewContextWithParams(1 << logn, _Q(pkg, qspec))
    return cQ, pkg.ring.CkksEncoder(cQ, max_batch, _root_table(1 << logn), options)


FUSED = [(4, "qi60:2", 1, 3), (4, "qi60:2", 2, 3), (4, "qi60:2", 8, 3), (10, "qi60:2", 512, 3), (10, "qi60:2", 4, 3), (13, "qi60:2", 1 << 12, 1),
         (14, "qi60:1", 1 << 13, 1)]


@pytest.mark.parametrize("logn,qspec,slots,batch", FUSED, ids=["N%d-%s-s%d" % (c[0], c[1].replace(":", ""), c[2]) for c in FUSED])
def test_fused_route_matches_the_restatement(gpu_pkg, oracle, monkeypatch, logn, qspec, slots, batch):
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    cQ, enc = _encoder(gpu_pkg, logn, qspec)
    assert enc.fused(slots)
    _, got = _check(oracle, gpu_pkg, enc, cQ, logn, qspec, slots, len(cQ.Modulus) - 1, 2.0 ** 40, batch)
    # the meaning: N / scale covers the rounding of at most N coefficients by 1/2 each, doubled for the double-precision FFTs
    for b in range(batch):
        assert np.max(np.abs(got[b] - _values(slots, b))) <= (1 << logn) / 2.0 ** 40


@pytest.mark.parametrize("logn,slots", [(6, 32), (6, 4), (4, 1)])
def test_fused_encode_as_one_kernel_from_batch_256(gpu_pkg, oracle, monkeypatch, logn, slots):
    """from 256 plaintexts on fused Encode is one kernel (a workgroup per plaintext does the scale-up too); below, an LDS kernel and a
    grid-wide scale-up: 256 and 255 plaintexts against the restatement and against the tiled route"""
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    qspec, batch, scale, level = "qi60:2", 256, 2.0 ** 40, 1
    cQ, enc = _encoder(gpu_pkg, logn, qspec, max_batch=batch)
    tiled = gpu_pkg.ring.CkksEncoder(cQ, batch, _root_table(1 << logn), gpu_pkg.ring.Options(ckks_encoder_tiled=1))
    assert enc.fused(slots) and not tiled.fused(slots)
    vals = np.stack([_values(slots, b) for b in range(batch)])
    pt = enc.Encode(cQ.NewPoly(batch), vals, level, scale)
    got = pt.get()
    r = _ref(oracle, gpu_pkg, logn, qspec)
    for b in (0, 1, 2, 100, 255):
        assert np.array_equal(got[b], r.encode(vals[b], level, scale)), b
    assert np.array_equal(tiled.Encode(cQ.NewPoly(batch), vals, level, scale).get(), got)
    assert np.array_equal(enc.Encode(cQ.NewPoly(batch - 1), vals[:-1], level, scale).get(), got[:-1])
    dec = enc.Decode(pt, slots, level, scale)
    assert np.array_equal(_bits(dec), _bits(tiled.Decode(pt, slots, level, scale)))
    assert np.array_equal(_bits(dec[255]), _bits(r.decode(got[255], slots, level, scale)))


@pytest.mark.parametrize("logn,slots", [(10, 512), (13, 1 << 12), (4, 8), (4, 1), (4, 2)])
def test_forced_tiled_route_gives_the_fused_bits(gpu_pkg, oracle, monkeypatch, logn, slots):
    """fused against tiled, the latter through lr_options::ckks_encoder_tiled and through LR_CKKS_ENCODER_TILED"""
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    qspec, batch, scale = "qi60:2", 3 if logn < 13 else 1, 2.0 ** 40
    cQ, fused = _encoder(gpu_pkg, logn, qspec)
    by_field = gpu_pkg.ring.CkksEncoder(cQ, MAX_BATCH, _root_table(1 << logn), gpu_pkg.ring.Options(ckks_encoder_tiled=1))
    monkeypatch.setenv("LR_CKKS_ENCODER_TILED", "1")
    by_env = gpu_pkg.ring.CkksEncoder(cQ, MAX_BATCH, _root_table(1 << logn))
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED")
    assert fused.fused(slots) and not by_field.fused(slots) and not by_env.fused(slots)
    pt, got = _check(oracle, gpu_pkg, by_field, cQ, logn, qspec, slots, 1, scale, batch)
    vals = np.stack([_values(slots, b) for b in range(batch)])
    for other in (fused, by_env):
        assert np.array_equal(other.Encode(cQ.NewPoly(batch), vals, 1, scale).get(), pt.get())
        assert np.array_equal(_bits(other.Decode(pt, slots, 1, scale)), _bits(got))


@pytest.mark.parametrize("logn,qspec,slots,batch", [(16, "qi60:2", 1 << 15, 2), (15, "qi60:1", 1 << 14, 1)], ids=["N16-s15", "N15-s14"])
def test_natural_tiled_route_matches_the_restatement(gpu_pkg, oracle, monkeypatch, logn, qspec, slots, batch):
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    cQ, enc = _encoder(gpu_pkg, logn, qspec)
    assert not enc.fused(slots) and enc.fused(1 << 13)
    _check(oracle, gpu_pkg, enc, cQ, logn, qspec, slots, len(cQ.Modulus) - 1, 2.0 ** 40, batch)


@pytest.mark.parametrize("qspec", ["qi60:1", "qi60:2", "qi60:6", "PN12QP109"])
def test_limbs_levels_and_batches(gpu_pkg, oracle, monkeypatch, qspec):
    """every level of the chain on a poly of all limbs (the upper limbs untouched), batches 1, 3 and max_batch, a sparse slot count"""
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    logn = 12 if qspec == "PN12QP109" else 8
    cQ, enc = _encoder(gpu_pkg, logn, qspec)
    L = len(cQ.Modulus)
    scale = 2.0 ** 30
    for level, batch, slots in [(L - 1, 1, 1 << (logn - 1)), (0, 3, 1 << (logn - 1)), (L // 2, MAX_BATCH, 16)]:
        _check(oracle, gpu_pkg, enc, cQ, logn, qspec, slots, level, scale, batch)
    # a poly of exactly level + 1 limbs
    if L > 1:
        vals = _values(32, 0)
        pt = enc.Encode(gpu_pkg.ring.Poly(cQ, L - 1, 1), vals, L - 2, scale)
        want = _ref(oracle, gpu_pkg, logn, qspec).encode(vals, L - 2, scale)
        assert np.array_equal(pt.get().reshape(L - 1, -1), want)
        assert np.array_equal(_bits(enc.Decode(pt, 32, L - 2, scale)[0]), _bits(_ref(oracle, gpu_pkg, logn, qspec).decode(want, 32, L - 2, scale)))


@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("logscale", [30, 40, 55])
def test_scales_and_both_branches_of_the_scale_up(gpu_pkg, oracle, monkeypatch, logscale, tiled):
    """coefficients chosen through the restatement's fft: positive ones up to 2^72 / scale (the big.Float branch above 2^64, the rounding of
    + 0.5 from 2^52), negative ones down to -2^62 / scale, exact integers and halves among them"""
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    logn, qspec, scale = 7, "qi60:2", 2.0 ** logscale
    N, r = 1 << logn, _ref(oracle, gpu_pkg, logn, qspec)
    cQ, enc = _encoder(gpu_pkg, logn, qspec, options=gpu_pkg.ring.Options(ckks_encoder_tiled=tiled))
    slots = N // 2
    rng = np.random.default_rng(logscale)
    re = 2.0 ** rng.uniform(40, 72, slots) / scale
    im = -(2.0 ** rng.uniform(0, 62, slots)) / scale
    re[:4] = np.array([2.0 ** 52, 2.0 ** 63, 2.0 ** 64 * (1 + 2.0 ** -40), 2.0 ** 66]) / scale
    vals = np.stack([r.fft(re, im), r.fft(np.floor(re * scale) / scale, np.ceil(im * scale) / scale), _values(slots, 0)])
    for v in vals[:2]:
        c = r.coefficients(v) * scale
        assert (c > 2.0 ** 64).sum() >= 4 and ((c > 2.0 ** 52) & (c < 2.0 ** 64)).sum() >= 4 and c.min() > -2.0 ** 63 and (c < -1).sum() >= 8
    _check(oracle, gpu_pkg, enc, cQ, logn, qspec, slots, 1, scale, 3, vals)


def _decode_both(gpu_pkg, oracle, logn, qspec, coeff_domain, slots, scale):
    """Decode of the plaintexts whose coefficient-domain image is given ([batch, limbs, N]): (fused route, restatement, tiled route)"""
    N, r = 1 << logn, _ref(oracle, gpu_pkg, logn, qspec)
    batch, L = coeff_domain.shape[0], coeff_domain.shape[1]
    cQ, enc = _encoder(gpu_pkg, logn, qspec)
    tiled = gpu_pkg.ring.CkksEncoder(cQ, MAX_BATCH, _root_table(N), gpu_pkg.ring.Options(ckks_encoder_tiled=1))
    assert enc.fused(slots) and not tiled.fused(slots)
    pt = cQ.NewPoly(batch).set(np.stack([r.cQ.ntt(c) for c in coeff_domain]))
    with np.errstate(all="ignore"):
        want = np.stack([r.decode_coeffs(c, slots, L - 1, scale) for c in coeff_domain])
    return enc.Decode(pt, slots, L - 1, scale), want, tiled.Decode(pt, slots, L - 1, scale)


@pytest.mark.parametrize("qspec,slots", [("qi60:1", 16), ("qi60:6", 16), ("qi60:6", 2), ("qi60:16", 16), ("PN12QP109", 8)])
def test_decode_of_uniformly_random_plaintexts(gpu_pkg, oracle, monkeypatch, qspec, slots):
    """at most 960 bits, so every value is finite: the whole multi-word CRT, the centring and the rounding"""
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    logn = 5
    Q = _Q(gpu_pkg, qspec)
    x = gpu_pkg.sampling.uniform_poly(Q, 1 << logn, 3, seed=len(Q) + slots).reshape(3, len(Q), 1 << logn)
    got, want, got_tiled = _decode_both(gpu_pkg, oracle, logn, qspec, x, slots, 2.0 ** 40)
    assert np.isfinite(want.view(np.float64)).all()
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(got_tiled), _bits(want))


def test_decode_at_the_centring_boundary_and_at_rounding_ties(gpu_pkg, oracle, monkeypatch):
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    logn, qspec = 5, "qi60:6"
    N, Q = 1 << logn, _Q(gpu_pkg, qspec)
    big = 1
    for q in Q:
        big *= q
    half = big >> 1
    tie = lambda k: (1 << k) + (1 << (k - 53))
    ints = [half - 1, half, half + 1, 0, 1, -1, big - 1, tie(53), tie(53) + 1, tie(64) - 1, tie(64), -tie(64), tie(100) + (1 << 47) * 2, tie(127), tie(128) - 1,
            tie(128), tie(128) + 1, -tie(192), (1 << 192) + 3 * (1 << 139), (1 << 256) - 1, -(1 << 256) + 1, tie(300), (1 << 53) - 1, 1 << 53, (1 << 64) - 1, 1 << 64,
            (1 << 128) - 1, 1 << 128, -(1 << 63), (1 << 320) + 1, half - tie(200), -half + 1]
    assert len(ints) == N
    rows = [ints, ints[::-1], [(-x) % big for x in ints]]
    x = np.array([[[int(v) % q for v in row] for q in Q] for row in rows], dtype=np.uint64)
    for slots in (N // 2, 1):
        got, want, got_tiled = _decode_both(gpu_pkg, oracle, logn, qspec, x, slots, 2.0 ** 30)
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(got_tiled), _bits(want)), slots
    # one slot reads coefficients 0 and N / 2 alone: the explicit expectation, without the restatement's CRT
    got, _, _ = _decode_both(gpu_pkg, oracle, logn, qspec, x[:1], 1, 1.0)
    assert got[0, 0].real == float(half - 1) and got[0, 0].imag == float(ref.centre(ints[N // 2], big))


def test_decode_above_two_to_the_1024_overflows_to_infinity(gpu_pkg, oracle, monkeypatch):
    """18 limbs of Qi60 (1080 bits): centred values from 2^1024 up are +-Inf as big.Float's Float64() makes them, and fft propagates them"""
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    logn, qspec = 4, "qi60:18"
    N, Q = 1 << logn, _Q(gpu_pkg, qspec)
    big = 1
    for q in Q:
        big *= q
    ints = [1 << 1024, -(1 << 1024), (1 << 1024) - (1 << 970), (1 << 1024) - (1 << 970) - 1, (1 << 1023), 5, -7, (big >> 1) - 1] + [3] * (N - 8)
    x = np.array([[[int(v) % q for v in ints] for q in Q]], dtype=np.uint64)
    got, want, got_tiled = _decode_both(gpu_pkg, oracle, logn, qspec, x, 1, 1.0)
    assert got[0, 0].real == math.inf and np.array_equal(got, want, equal_nan=True) and np.array_equal(got_tiled, want, equal_nan=True)
    cQ, enc = _encoder(gpu_pkg, logn, qspec)
    r = _ref(oracle, gpu_pkg, logn, qspec)
    for shift in range(1, 8):                                       # each of the special values at coefficient 0, a finite one at N / 2
        row = ints[shift:shift + 1] + [0] * (N // 2 - 1) + [9] + [0] * (N // 2 - 1)
        c = np.array([[int(v) % q for v in row] for q in Q], dtype=np.uint64)
        g = enc.Decode(cQ.NewPoly(1).set(r.cQ.ntt(c)[None]), 1, len(Q) - 1, 1.0)[0, 0]
        assert g.real == ref.scale_down(ref.centre(row[0], big), 1.0) and g.imag == 9.0, shift
    full = enc.Decode(cQ.NewPoly(1).set(r.cQ.ntt(x[0])[None]), N // 2, len(Q) - 1, 2.0 ** 40)
    with np.errstate(all="ignore"):
        assert np.array_equal(full[0], r.decode_coeffs(x[0], N // 2, len(Q) - 1, 2.0 ** 40), equal_nan=True)


@pytest.mark.parametrize("tiled", [0, 1])
def test_device_pointer_entry_points(gpu_pkg, tiled, monkeypatch):
    """slot values in device memory (here: one-limb polys used as plain buffers) against the host-value calls"""
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    logn, qspec, batch, slots, scale = 10, "qi60:2", 3, 256, 2.0 ** 40
    N = 1 << logn
    ring = gpu_pkg.ring
    cQ, enc = _encoder(gpu_pkg, logn, qspec, options=ring.Options(ckks_encoder_tiled=tiled))
    vals = np.stack([_values(slots, b) for b in range(batch)])
    src, dst = ring.Poly(cQ, 1, batch), ring.Poly(cQ, 1, batch)
    flat = np.zeros(batch * N, dtype=np.uint64)
    flat[:batch * slots * 2] = vals.view(np.uint64).reshape(-1)                        # [batch][slots] is dense
    src.set(flat.reshape(batch, 1, N))
    pt_host = enc.Encode(cQ.NewPoly(batch), vals, 1, scale)
    pt_dev = enc.EncodeDevice(cQ.NewPoly(batch), src.device_ptr, slots, 1, scale, batch)
    assert np.array_equal(pt_dev.get(), pt_host.get())
    dst.set(np.zeros((batch, 1, N), dtype=np.uint64))
    enc.DecodeDevice(pt_dev, slots, 1, scale, dst.device_ptr)
    cQ.Sync()
    got = dst.get().reshape(-1)
    assert np.array_equal(got[:batch * slots * 2], _bits(enc.Decode(pt_host, slots, 1, scale)).reshape(-1)) and not got[batch * slots * 2:].any()


@pytest.mark.parametrize("logn", [3, 4, 11])
def test_tables(gpu_pkg, logn):
    N = 1 << logn
    cQ, enc = _encoder(gpu_pkg, logn, "qi60:1")
    rot, roots = enc.tables()
    assert np.array_equal(rot, ref.rot_group(N)) and np.array_equal(_bits(roots), _bits(_root_table(N)))
    # no table given: the library's own, from the same expression with the host libm (the last place may differ from Python's build of it)
    rot, roots = gpu_pkg.ring.CkksEncoder(cQ).tables()
    assert np.array_equal(rot, ref.rot_group(N)) and roots[2 * N] == roots[0] == 1 and np.max(np.abs(roots - _root_table(N))) < 4e-16


def test_refusals(gpu_pkg):
    logn, N = 8, 1 << 8
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    Q = _Q(gpu_pkg, "qi60:3")
    cQ, other = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, Q)

    def err(f, *args):
        with pytest.raises(nat.LatticeRingError) as e:
            f(*args)
        return e.value
    assert err(ring.CkksEncoder, cQ, 0).code == 4 and err(ring.CkksEncoder, cQ, 65536).code == 4
    # 35 limbs of 60 bits exceed the 32 words of the decoder's CRT
    assert err(ring.CkksEncoder, ring.NewContextWithParams(16, _Q(gpu_pkg, "qi60:35"))).code == 4
    enc = ring.CkksEncoder(cQ, 2, _root_table(N))
    v, s = np.zeros((1, 8), dtype=np.complex128), 2.0 ** 30
    for bad in (3, 12, N):                                                                              # not a power of two, above N / 2
        assert err(enc.Encode, cQ.NewPoly(), np.zeros((1, bad), dtype=np.complex128), 2, s).code == 4
        assert err(enc.Decode, cQ.NewPoly(), bad, 2, s).code == 4
        assert err(enc.fused, bad).code == 4
    assert err(enc.Decode, cQ.NewPoly(), 0, 2, s).code == 4 and err(enc.Decode, cQ.NewPoly(), -4, 2, s).code == 4
    for bad_scale in (0.0, -1.0, math.inf, math.nan):
        assert err(enc.Encode, cQ.NewPoly(), v, 2, bad_scale).code == 4 and err(enc.Decode, cQ.NewPoly(), 8, 2, bad_scale).code == 4
    assert err(enc.Encode, cQ.NewPoly(2), v, 2, s).code == 3                                            # batch != the poly's
    assert err(enc.Encode, cQ.NewPoly(3), np.zeros((3, 8), dtype=np.complex128), 2, s).code == 3        # batch > max_batch
    assert err(enc.Decode, cQ.NewPoly(3), 8, 2, s).code == 3
    assert err(enc.Encode, other.NewPoly(), v, 2, s).code == 4                                          # a poly of another context
    assert err(enc.Decode, other.NewPoly(), 8, 2, s).code == 4
    assert err(enc.Encode, ring.Poly(cQ, 2, 1), v, 2, s).code == 3                                      # fewer than level + 1 limbs
    assert err(enc.Decode, ring.Poly(cQ, 2, 1), 8, 2, s).code == 3
    assert err(enc.Encode, cQ.NewPoly(), v, 3, s).code == 3 and err(enc.Decode, cQ.NewPoly(), 8, -1, s).code == 3      # no such level
    L, pt = nat.lib(), cQ.NewPoly()
    buf = np.zeros(4 * N + 2, dtype=np.float64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    for rc in (L.lr_ckks_encode(None, ptr, 8, 2, s, 1, pt.h), L.lr_ckks_encode(enc.h, None, 8, 2, s, 1, pt.h), L.lr_ckks_encode(enc.h, ptr, 8, 2, s, 1, None),
               L.lr_ckks_decode(enc.h, None, 8, 2, s, 1, ptr), L.lr_ckks_decode(enc.h, pt.h, 8, 2, s, 1, None), L.lr_ckks_decode(None, pt.h, 8, 2, s, 1, ptr),
               L.lr_ckks_encode_device(enc.h, None, 8, 2, s, 1, pt.h), L.lr_ckks_decode_device(enc.h, pt.h, 8, 2, s, 1, None),
               L.lr_ckks_encoder_tables(enc.h, None, None), L.lr_ckks_encoder_route(enc.h, 8, None), L.lr_ckks_encoder_route(None, 8, C.byref(C.c_int())),
               L.lr_ckks_encoder_create(None, 1, None, C.byref(C.c_void_p())), L.lr_ckks_encoder_create(cQ.h, 1, None, None)):
        assert rc == 4
    assert L.lr_ckks_encoder_destroy(None) == 0
    # the handle stays usable after its refusals
    vals = _values(8, 0)
    assert np.max(np.abs(enc.Decode(enc.Encode(pt, vals, 2, s), 8, 2, s)[0] - vals)) <= N / s


def test_encode_encrypt_decrypt_decode(gpu_pkg, oracle, monkeypatch):
    """Encode -> lr_ckks_encrypt_pk -> lr_ckks_decrypt -> Decode with fixed u and e: the restatement over the oracle's encrypt and decrypt,
    bit for bit, and the slot values back within N / scale plus the fresh-noise bound of tests/test_gpu_ckks_semantics.py (2^12 per
    coefficient, N coefficients, roots of modulus 1)"""
    monkeypatch.delenv("LR_CKKS_ENCODER_TILED", raising=False)
    logn, nq, np_, batch, scale = 10, 4, 2, 2, 2.0 ** 40
    N, slots = 1 << logn, 1 << (logn - 1)
    _, Qf, Pf = gpu_pkg.params.ckks_moduli("PN15QP880")
    Q, P = Qf[:nq], Pf[:np_]
    QP, level = Q + P, nq - 1
    ocQP, ocQ, ocP = oracle.Context(N, QP), oracle.Context(N, Q), oracle.Context(N, P)
    oplan = oracle.CkksPlan(ocQ, ocP)
    ring = gpu_pkg.ring
    cQ, cP, cQP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, QP)
    plan = ring.CkksPlan(cQ, cP, batch)
    enc = ring.CkksEncoder(cQ, batch, _root_table(N))
    r = ref.Encoder(oracle, N, Q, _root_table(N))
    s_ntt = ocQP.ntt(_residues(_small(N, 1, 31), QP))
    a_pk = gpu_pkg.sampling.uniform_poly(QP, N, 1, seed=1000)[0]
    e_pk = ocQP.ntt(_residues(_small(N, 6, 1001), QP))
    pk0 = _mont(np.array([[(int(e) - int(a) * int(s)) % q for a, s, e in zip(a_pk[i], s_ntt[i], e_pk[i])] for i, q in enumerate(QP)], dtype=np.uint64), QP)   # -a s + e
    pk1 = _mont(a_pk, QP)
    sk = _mont(s_ntt[:nq], Q)
    u = np.stack([_mont(ocQP.ntt(_residues(_small(N, 1, 40 + b), QP)), QP) for b in range(batch)])
    e0 = np.stack([_residues(_small(N, 6, 50 + b), QP) for b in range(batch)])
    e1 = np.stack([_residues(_small(N, 6, 60 + b), QP) for b in range(batch)])
    vals = np.stack([_values(slots, b) for b in range(batch)])
    pt = enc.Encode(cQ.NewPolyLvl(level, batch), vals, level, scale)
    ct = (cQ.NewPolyLvl(level, batch), cQ.NewPolyLvl(level, batch))
    QPpoly = lambda x: cQP.NewPoly(x.shape[0]).set(x)
    plan.EncryptPk(level, QPpoly(u), (QPpoly(pk0[None]), QPpoly(pk1[None])), (QPpoly(e0), QPpoly(e1)), pt, ct)
    out = cQ.NewPolyLvl(level, batch)
    plan.Decrypt(level, ct, cQ.NewPoly(1).set(sk[None]), out)
    got = enc.Decode(out, slots, level, scale)
    for b in range(batch):
        want_ct = oplan.encrypt_pk(ocQP, level, u[b], pk0, pk1, e0[b], e1[b], r.encode(vals[b], level, scale))
        want = r.decode(oplan.decrypt(level, np.stack([want_ct[0], want_ct[1]]), sk), slots, level, scale)
        assert np.array_equal(_bits(got[b]), _bits(want)), b
        assert np.max(np.abs(got[b] - vals[b])) <= N / scale + N * (1 << 12) / scale, b
