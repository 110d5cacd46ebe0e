"""Emulator harness of the assembly NTT kernels (test infrastructure: imports the oracle).

Runs one workgroup of a generated instruction stream (asmgen/gen_ntt.py, gen_intt.py) on the numpy SIMT emulator of
asmgen/isa.py and compares it with the CPU oracle: the same checks the device tests make, without a GPU.

    python tests/asm_emulate.py 15 --selftest [threads]          # forward kernels of 2^15
    python tests/asm_emulate.py 15 --selftest-inverse [threads]
    python tests/asm_emulate.py 16 --selftest | --selftest-inverse   # the 2^15 sub-block kernels of N = 2^16
    python tests/asm_emulate.py 15 --selftest | --selftest-inverse --halves      # the 2^14 sub-block kernels of N = 2^15
    python tests/asm_emulate.py 15 --selftest-persist                # the persistent forward kernels of the diagnostics build

Every generator comes from asmgen/catalogue.py (make); --list-cases after any of these prints the catalogue keys its cases exercise
instead of running them.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lattigo-fhe-by-go_amd", "csrc", "asmgen"))

import catalogue  # noqa: E402
from gen_ntt import FP_LIMIT  # noqa: E402
from isa import Machine, Program  # noqa: E402,F401

sys.path.insert(0, os.path.join(ROOT, "tests"))
import limit_moduli as lm  # noqa: E402


# ------------------------------------------------------------------------------------------
# self test on the numpy emulator
# ------------------------------------------------------------------------------------------
def emulate(gen, inverse=False, q=None, geom=None, x=None):
    # geom = (x, y, z, hole, group, rows per poly): workgroup ids and the digit-group arguments of NttLaunch
    """run one workgroup of the generated program on the numpy emulator; returns (bit-exact?, summary text).
    x: the input vector (any 64-bit values forward, [0, 4q) inverse) instead of the seeded random one"""
    import numpy as np

    from isa import Machine
    sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), "..", "..", ".."))
    import __graft_entry__ as graft
    oracle = graft.load_oracle()
    pkg = graft.load_package()
    logn = gen.logn
    N = 1 << logn
    q = q or pkg.params.Qi60()[-3]
    oc = oracle.Context(N, [q])
    given = x
    x = pkg.sampling.random_u64((N,), seed=5)                 # full 64-bit inputs
    x[:4] = np.uint64(0xFFFFFFFFFFFFFFFF)
    if inverse:
        x = (x % np.uint64(4 * q)).astype(np.uint64)          # the inverse accepts [0, 4q)
        x[:4] = np.uint64(4 * q - 1)
    if given is not None:
        x = np.array(given, dtype=np.uint64).reshape(N).copy()
        assert not inverse or int(x.max()) < 4 * q
    canon = np.array([[int(val) % q for val in x]], dtype=np.uint64)
    want = (oc.intt(canon) if inverse else oc.ntt(canon))[0]

    # host-side tables exactly as lr_abi_core.cpp builds them
    table = oc.ntt_psi_inv[0] if inverse else oc.ntt_psi[0]
    psi = [int(oracle.inv_mform(int(w), q)) for w in table]
    n_inv = pow(N, -1, q)
    if inverse:
        psi[0] = psi[1] * n_inv % q                           # constant of the fused last stage
    tw = np.zeros((N, 2), dtype=np.uint64)
    for i, w in enumerate(psi):
        tw[i, 0] = w
        tw[i, 1] = (w << 64) // q
    blocks = N // 16
    twf = np.zeros((15, blocks, 2), dtype=np.uint64)
    for cc in range(4):
        for j in range(1 << cc):
            for bk in range(blocks):
                twf[(1 << cc) - 1 + j, bk] = tw[((blocks + bk) << cc) + j]
    qh = (q >> 32) + 1
    g = qh.bit_length() - 1
    red_m = min((1 << (32 + g)) // qh, 0xFFFFFFFF)
    lp = np.zeros(8, dtype=np.uint64)
    lp[0] = q
    lp[2] = (1 << 128) // q >> 64
    lp[5] = n_inv
    lp[6] = (n_inv << 64) // q
    lp[7] = red_m | (g << 32)

    # flat memory image (byte addresses)
    def place(arr, addr):
        words = np.ascontiguousarray(arr).view(np.uint32).ravel()
        mem[addr // 4: addr // 4 + words.size] = words

    gx, gy, gz, hole, group, rows = (geom or (0, 0, 0, 0, 0, 1))[:6]
    item = gx + (hole if gx >= gz * hole else 0)
    where = ((gz * group + gy) * rows + item) * 8 * N          # byte offset of the addressed row
    span = ((gz * group + gy + 1) * rows + 1) * 8 * N
    A_KARG, A_IN = 0x800, 0x1000
    A_OUT = A_IN + span
    A_LP = A_OUT + span
    A_TW = A_LP + 0x1000
    A_TWF = A_TW + 16 * N + 0x1000
    A_FTW = A_TWF + 16 * 15 * blocks + 0x1000
    A_FTWF = A_FTW + 16 * N + 0x1000
    A_FLP = A_FTWF + 16 * 15 * blocks + 0x1000
    A_STAMPS = A_FLP + 0x1000                                   # timeline builds: NttLaunch::epi_x
    mem = np.zeros((A_STAMPS + 0x2000) // 4, dtype=np.uint32)
    place(x, A_IN + where)
    place(lp, A_LP)
    place(tw, A_TW)
    place(twf, A_TWF)
    fp_tables(np, q, n_inv, tw, twf, lambda a, b, c: (place(a, A_FTW), place(b, A_FTWF), place(c, A_FLP)))
    karg = np.zeros(22, dtype=np.uint64)
    karg[13], karg[14], karg[15] = A_FTW - A_TW, A_FTWF - A_TWF, A_FLP
    if getattr(gen, "epi", False):
        # x and plus: canonical polys laid out like the output; c: a random constant in (w, w / q) form on an FP64 limb, as the Shoup
        # pair (w, floor(w 2^64 / q)) on an integer one
        rng = np.random.default_rng(7)
        xe = (rng.integers(0, 1 << 62, N, dtype=np.uint64) % np.uint64(q)).astype(np.uint64)
        pe = (rng.integers(0, 1 << 62, N, dtype=np.uint64) % np.uint64(q)).astype(np.uint64)
        xe[:3], pe[:3] = [0, q - 1, q - 1], [q - 1, 0, q - 1]
        ce = int(rng.integers(1, q))
        A_X, A_P, A_EC = mem.size * 4, mem.size * 4 + span, mem.size * 4 + 2 * span
        mem = np.concatenate([mem, np.zeros((2 * span + 0x1000) // 4, dtype=np.uint32)])
        place(xe, A_X + where)
        place(pe, A_P + where)
        if q < FP_LIMIT and getattr(gen, "gf", None) is not None:      # a dual kernel runs this limb on its FP64 body
            place(np.array([ce, np.float64(ce) / np.float64(q)], dtype=np.float64), A_EC)      # modulus index 0
        else:
            place(np.array([ce, (ce << 64) // q], dtype=np.uint64), A_EC)
        karg[16], karg[17], karg[18], karg[19], karg[20] = A_X, rows * N, A_P, rows * N, A_EC
        want = np.array([((int(a) - int(b)) * ce + int(c)) % q for a, b, c in zip(xe, want, pe)], dtype=np.uint64)
    karg[0], karg[1], karg[2], karg[3] = A_IN, A_OUT, rows * N, rows * N
    karg[4] = 0 | (1 << 32)        # in_limb0, in_limb_step
    karg[5] = 0 | (1 << 32)        # out_limb0, out_limb_step
    karg[6] = 0 | (0 << 32)        # mod0, mod_step: one modulus serves every row of this harness
    karg[11] = 0 | (hole << 32)    # sub_log, hole
    karg[12] = group               # group, pad
    n_items = geom[6] if geom and len(geom) > 6 else gx + 1   # (a seventh entry: fewer items than x + 1 -- a workgroup of the padded grid)
    karg[7] = n_items | (1 << 32)  # n_items, batch
    karg[8], karg[9], karg[10] = A_LP, A_TW, A_TWF
    if getattr(gen, "profile", False):
        karg[16] = A_STAMPS
    place(karg, A_KARG)

    prog = gen.build()
    m = Machine(gen.T, 160 * 1024, mem.size)
    m.mem = mem
    m.vgpr[0] = np.arange(gen.T, dtype=np.uint32)
    m.vdef[0] = True
    m.sgpr[0], m.sgpr[1] = A_KARG, 0
    m.sgpr[gen.WGX.idx], m.sgpr[gen.WGY.idx], m.sgpr[4] = gx, gy, gz
    m.sdef[0:5] = True
    m.count_lds = bool(__import__("os").environ.get("LR_EMU_LDS_STATS"))
    m.run(prog)
    got = m.mem[(A_OUT + where) // 4: (A_OUT + where) // 4 + 2 * N].view(np.uint64)
    if n_items <= gx:                                          # a workgroup of the padded grid: leaves at once, its row stays untouched
        want = np.zeros(N, dtype=np.uint64)
        assert sum(n for op, n in m.executed.items() if op.startswith(("global_store", "ds_"))) == 0
    ok = np.array_equal(got, want)
    if m.count_lds:
        gen.lds_stats = m.lds_stats
        gen.last_prog = prog
    cnt = prog.count()
    valu = sum(n for op, n in cnt.items() if op.startswith("v_"))
    bf = (1 << gen.A) * logn // 2
    info = "%d instructions, %d VALU = %.1f per butterfly, s_nop %d" % (len(prog.ins), valu, valu / bf, cnt.get("s_nop", 0))
    if getattr(gen, "gf", None) is not None:
        ran = sum(n for op, n in m.executed.items() if op.startswith("v_"))
        info = "%s body, %d VALU executed = %.1f per butterfly" % ("FP64" if m.executed.get("v_fma_f64") else "integer", ran, ran / bf)
        ok = ok and bool(m.executed.get("v_fma_f64")) == (q < FP_LIMIT)
    if not ok:
        bad = np.nonzero(got != want)[0]
        info += "\n  mismatches: %d first: %s %s %s" % (bad.size, bad[:8], [hex(int(got[i])) for i in bad[:3]],
                                                       [hex(int(want[i])) for i in bad[:3]])
    return ok, info




def emulate_persist(make_gen, q, polys, per_wg, chunk):
    """forward persistent kernel: the workgroup of chunk `chunk` transforms polys [chunk * per_wg, min(polys, (chunk + 1) * per_wg)) of a
    batch of `polys` one-limb polys in its loop; every output row of the batch is compared (rows of other chunks must stay zero)"""
    import numpy as np

    from isa import Machine
    import __graft_entry__ as graft
    oracle = graft.load_oracle()
    pkg = graft.load_package()
    gen = make_gen()
    logn = gen.logn
    N = 1 << logn
    q = q or pkg.params.Qi60()[-3]
    oc = oracle.Context(N, [q])
    x = pkg.sampling.random_u64((polys, N), seed=21)
    x[:, :4] = np.uint64(0xFFFFFFFFFFFFFFFF)
    want = np.zeros((polys, N), dtype=np.uint64)
    lo, hi = chunk * per_wg, min(polys, (chunk + 1) * per_wg)
    for b in range(lo, hi):
        want[b] = oc.ntt(np.array([[int(val) % q for val in x[b]]], dtype=np.uint64))[0]
    psi = [int(oracle.inv_mform(int(w), q)) for w in oc.ntt_psi[0]]
    n_inv = pow(N, -1, q)
    tw = np.zeros((N, 2), dtype=np.uint64)
    for i, w in enumerate(psi):
        tw[i, 0] = w
        tw[i, 1] = (w << 64) // q
    blocks = N // 16
    twf = np.zeros((15, blocks, 2), dtype=np.uint64)
    for cc in range(4):
        for j in range(1 << cc):
            for bk in range(blocks):
                twf[(1 << cc) - 1 + j, bk] = tw[((blocks + bk) << cc) + j]
    lp = np.zeros(8, dtype=np.uint64)
    lp[0] = q
    lp[2] = (1 << 128) // q >> 64
    lp[5] = n_inv
    lp[6] = (n_inv << 64) // q
    stride_in, stride_out = 2 * N, 3 * N          # polys further apart than their rows, and differently on the two sides
    A_KARG, A_IN = 0x800, 0x1000
    A_OUT = A_IN + 8 * stride_in * polys + 0x1000
    A_LP = A_OUT + 8 * stride_out * polys + 0x1000
    A_TW = A_LP + 0x1000
    A_TWF = A_TW + 16 * N + 0x1000
    A_FTW = A_TWF + 16 * 15 * blocks + 0x1000
    A_FTWF = A_FTW + 16 * N + 0x1000
    A_FLP = A_FTWF + 16 * 15 * blocks + 0x1000
    A_STAMPS = A_FLP + 0x1000
    mem = np.zeros((A_STAMPS + 0x4000) // 4, dtype=np.uint32)

    def place(arr, addr):
        words = np.ascontiguousarray(arr).view(np.uint32).ravel()
        mem[addr // 4: addr // 4 + words.size] = words

    for b in range(polys):
        place(x[b], A_IN + 8 * stride_in * b)
    place(lp, A_LP)
    place(tw, A_TW)
    place(twf, A_TWF)
    fp_tables(np, q, n_inv, tw, twf, lambda a, b, c: (place(a, A_FTW), place(b, A_FTWF), place(c, A_FLP)))
    karg = np.zeros(22, dtype=np.uint64)
    karg[13], karg[14], karg[15] = A_FTW - A_TW, A_FTWF - A_TWF, A_FLP
    karg[0], karg[1], karg[2], karg[3] = A_IN, A_OUT, stride_in, stride_out
    karg[4] = 0 | (1 << 32)
    karg[5] = 0 | (1 << 32)
    karg[6] = 0
    karg[7] = 1 | (polys << 32)        # n_items, batch
    karg[8], karg[9], karg[10] = A_LP, A_TW, A_TWF
    karg[11] = 0                       # sub_log, hole
    karg[12] = polys | (per_wg << 32)  # group (= batch for a plain launch), fuse_top = polys per workgroup
    if getattr(gen, "profile", False):
        karg[16] = A_STAMPS
    place(karg, A_KARG)
    prog = gen.build()
    m = Machine(gen.T, 160 * 1024, mem.size)
    m.mem = mem
    m.vgpr[0] = np.arange(gen.T, dtype=np.uint32)
    m.vdef[0] = True
    m.sgpr[0], m.sgpr[1] = A_KARG, 0
    m.sgpr[gen.WGX.idx], m.sgpr[gen.WGY.idx], m.sgpr[4] = 0, chunk, 0
    m.sdef[0:5] = True
    m.run(prog)
    got = np.stack([m.mem[(A_OUT + 8 * stride_out * b) // 4: (A_OUT + 8 * stride_out * b) // 4 + 2 * N].view(np.uint64) for b in range(polys)])
    ok = bool(np.array_equal(got, want))
    ran = sum(n for op, n in m.executed.items() if op.startswith("v_"))
    info = "%d polys in the loop, %d VALU executed = %.1f per poly, at most %d vector-memory operations in flight" % (
        hi - lo, ran, ran / (hi - lo), m.max_vm_outstanding)
    if getattr(gen, "gf", None) is not None:
        ok = ok and bool(m.executed.get("v_fma_f64")) == (q < FP_LIMIT)
    if not ok:
        bad = np.argwhere(got != want)
        info += "\n  mismatches: %d first: %s" % (len(bad), bad[:4].tolist())
    return ok, info


def persist_cases(threads=1024):
    cases = [("mode %d" % mode, mode, {}, test_moduli(15, mode)[0]) for mode in (0, 1, 2)]
    cases += [("dual", 3, {}, q) for q in fp_test_moduli(15)]
    cases.append(("dual timeline", 3, {"profile": True}, fp_test_moduli(15)[0]))
    out = []
    for name, mode, flavour, q in cases:
        # three polys in one loop (prefetch taken twice, skipped once); a trailing chunk of one poly (no prefetch at all)
        for polys, per_wg, chunk in ((3, 3, 0), (3, 2, 1)):
            run = lambda mk, q=q, shape=(polys, per_wg, chunk): emulate_persist(mk, q, *shape)
            out.append(("forward persistent logN=15 %s %s, chunk %d of %d x %d" % (name, bits(q), chunk, polys, per_wg),
                        [(("fwd", mode, 15, threads, dict(flavour, persist=True)), run)], VERDICT))
    return out


def fp_tables(np, q, n_inv, tw, twf, put):
    """what lr_abi_core.cpp builds for the FP body: every (w, floor(w 2^64 / q)) becomes the pair of doubles (w, RN(w / q));
    FpLimb = {q, RN(1/q), N^-1 mod q, RN(N^-1 / q)}, all zero for a modulus the FP body does not take"""
    def conv(t):
        w = t[..., 0].astype(np.float64)
        out = np.zeros(t.shape, dtype=np.float64)
        out[..., 0] = w
        out[..., 1] = w / np.float64(q)
        return out
    flp = np.zeros(4, dtype=np.float64)
    if q < FP_LIMIT:
        flp[:] = [q, np.float64(1.0) / np.float64(q), n_inv, np.float64(n_inv) / np.float64(q)]
        put(conv(tw), conv(twf), flp)
    else:
        put(np.zeros(tw.shape), np.zeros(twf.shape), flp)


def test_moduli(logn, mode):
    """moduli at both ends of the range the mode accepts (tests/limit_moduli.py): the largest NTT prime below the mode's limit first,
    the smallest above 2^33 (the 32-bit Barrett constant's limit) last; mode 1 also takes the headline modulus and the smallest prime
    above 2^57, where mode 2 hands over to it"""
    sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), "..", "..", ".."))
    import __graft_entry__ as graft
    params = graft.load_package().params
    lo = lm.above(33, logn)
    if mode == 2:
        return [lm.below(57, logn), lo]
    if mode == 1:
        return [params.Qi60()[-3], lm.below(60, logn), lm.above(57, logn), lo]
    return [lm.below(61, logn), lm.above(60, logn), lo]


_STRESS = {}


def stress_inputs(logn, q, inverse):
    """[(family, input vector or None)]: the seeded random input of emulate / emulate_sub (None) and the stress polys of
    tests/limit_moduli.py for a transform of 2^logn -- all of them up to 2^13, the three harshest beyond (run time)"""
    import numpy as np
    key = (logn, q, inverse)
    if key not in _STRESS:
        import __graft_entry__ as graft
        oc = graft.load_oracle().Context(1 << logn, [q])
        names, x = lm.stress_polys([q], 1 << logn, "intt" if inverse else "ntt", oc, families=None if logn <= 13 else lm.harshest(logn))
        assert set(lm.harshest(logn)) <= set(names)
        _STRESS[key] = [("random", None)] + [(n, np.ascontiguousarray(x[k, 0])) for k, n in enumerate(names)]
    return _STRESS[key]


def over_families(logn, q, inverse, run, harshest_only=False):
    """run(x) -> (ok, info) for every stress input (harshest_only: the random one and the three harshest -- a second addressing of a
    case that has already run them all); returns (all ok, info of the last run + the families that failed)"""
    good, info, bad = True, "", []
    fams = stress_inputs(logn, q, inverse)
    if harshest_only:
        fams = [f for f in fams if f[0] == "random" or f[0] in lm.harshest(logn)]
    for name, x in fams:
        ok, info = run(x)
        if not ok:
            good = False
            bad.append(name + ": " + info)
    info = "%d inputs; %s" % (len(fams), info.split("\n")[0])
    return good, info + "".join("\n  FAILED on " + b for b in bad)


def fp_test_moduli(logn):
    """dual kernels: the largest NTT prime below 2^46 (the FP body's range bounds at their tightest), a 30-bit one (below what the
    integer bodies accept) and one just above 2^46 (integer body of the same kernel)"""
    sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), "..", "..", ".."))
    import __graft_entry__ as graft
    params = graft.load_package().params
    step = 2 << logn
    p = FP_LIMIT - step + 1
    while not params.is_prime(p):
        p -= step
    return [p, params.GenerateNTTPrimes(30, logn, 1)[0], params.GenerateNTTPrimes(46, logn, 1)[0]]


def emulate_sub(make_gen, inverse, q, pretop=False, order=(0, 1), x=None):
    """N = 2^16 through the two sub-block workgroups of one limb; returns (bit-exact?, summary).  x: the input vector, as in emulate"""
    import numpy as np

    from isa import Machine
    sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), "..", "..", ".."))
    import __graft_entry__ as graft
    oracle = graft.load_oracle()
    pkg = graft.load_package()
    N = 1 << make_gen().logn
    NF = 2 * N
    oc = oracle.Context(NF, [q])
    given = x
    x = pkg.sampling.random_u64((NF,), seed=9)
    x[:4] = np.uint64(0xFFFFFFFFFFFFFFFF)
    if inverse:
        x = (x % np.uint64(4 * q)).astype(np.uint64)
    if given is not None:
        x = np.array(given, dtype=np.uint64).reshape(NF).copy()
        assert not inverse or int(x.max()) < 4 * q
    canon = np.array([[int(val) % q for val in x]], dtype=np.uint64)
    want = (oc.intt(canon) if inverse else oc.ntt(canon))[0]
    table = oc.ntt_psi_inv[0] if inverse else oc.ntt_psi[0]
    psi = [int(oracle.inv_mform(int(w), q)) for w in table]
    n_inv = pow(NF, -1, q)
    psi[0] = psi[1] * n_inv % q if inverse else q - psi[1]     # lr_abi_core.cpp fills the unused heap entry 0 like this
    tw = np.zeros((NF, 2), dtype=np.uint64)
    for i, w in enumerate(psi):
        tw[i, 0] = w
        tw[i, 1] = (w << 64) // q
    blocks = NF // 16
    twf = np.zeros((15, blocks, 2), dtype=np.uint64)
    for cc in range(4):
        for j in range(1 << cc):
            for bk in range(blocks):
                twf[(1 << cc) - 1 + j, bk] = tw[((blocks + bk) << cc) + j]
    lp = np.zeros(8, dtype=np.uint64)
    lp[0] = q
    lp[2] = (1 << 128) // q >> 64
    lp[5] = n_inv
    lp[6] = (n_inv << 64) // q
    A_KARG, A_IN = 0x800, 0x1000
    A_OUT = A_IN + 8 * NF + 0x1000
    A_LP = A_OUT + 8 * NF + 0x1000
    A_TW = A_LP + 0x1000
    A_TWF = A_TW + 16 * NF + 0x1000
    A_FTW = A_TWF + 16 * 15 * blocks + 0x1000
    A_FTWF = A_FTW + 16 * NF + 0x1000
    A_FLP = A_FTWF + 16 * 15 * blocks + 0x1000
    mem = np.zeros((A_FLP + 0x1000) // 4, dtype=np.uint32)

    def place(arr, addr):
        words = np.ascontiguousarray(arr).view(np.uint32).ravel()
        mem[addr // 4: addr // 4 + words.size] = words

    if pretop:
        # what ntt_top_kernel leaves for the plain forward sub-blocks: X = U + V*psi[1], Y = U - V*psi[1] (lazy, < 8q)
        xs = [int(a) % q for a in x]
        w = psi[1]
        x = np.array([(xs[j] + xs[j + N] * w) % q + q for j in range(N)] + [(xs[j] - xs[j + N] * w) % q + 3 * q for j in range(N)],
                     dtype=np.uint64)
    place(x, A_IN)
    place(lp, A_LP)
    place(tw, A_TW)
    place(twf, A_TWF)
    fp_tables(np, q, n_inv, tw, twf, lambda a, b, c: (place(a, A_FTW), place(b, A_FTWF), place(c, A_FLP)))
    karg = np.zeros(22, dtype=np.uint64)
    karg[13], karg[14], karg[15] = A_FTW - A_TW, A_FTWF - A_TWF, A_FLP
    karg[0], karg[1], karg[2], karg[3] = A_IN, A_OUT, NF, NF
    karg[4] = 0 | (1 << 32)
    karg[5] = 0 | (1 << 32)
    karg[6] = 0
    karg[7] = 1 | (1 << 32)
    karg[8], karg[9], karg[10] = A_LP, A_TW, A_TWF
    karg[11] = 1                   # sub_log = 1, hole = 0
    karg[12] = 1                   # group
    fuse_last = getattr(make_gen(), "fuse_last", False)
    if fuse_last:
        # inverse with the fused last stage: the launch's pair flags (one u32 per wave of a limb's two sub-blocks), zeroed by the host
        A_FLAGS = mem.size * 4
        mem = np.concatenate([mem, np.zeros(0x1000 // 4, dtype=np.uint32)])
        karg[16] = A_FLAGS
    if getattr(make_gen(), "epi", False):
        # the epilogue of the plain forward sub-blocks: out = (x - NTT(in)) * c + plus, x / plus laid out like the output
        rng = np.random.default_rng(11)
        xe = (rng.integers(0, 1 << 62, NF, dtype=np.uint64) % np.uint64(q)).astype(np.uint64)
        pe = (rng.integers(0, 1 << 62, NF, dtype=np.uint64) % np.uint64(q)).astype(np.uint64)
        xe[:3], pe[:3] = [0, q - 1, q - 1], [q - 1, 0, q - 1]
        xe[N:N + 3], pe[N:N + 3] = [q - 1, 0, q - 1], [0, q - 1, q - 1]
        ce = int(rng.integers(1, q))
        A_X = mem.size * 4
        A_P, A_EC = A_X + 8 * NF + 0x1000, A_X + 16 * NF + 0x2000
        mem = np.concatenate([mem, np.zeros((16 * NF + 0x3000) // 4, dtype=np.uint32)])
        place(xe, A_X)
        place(pe, A_P)
        if q < FP_LIMIT and getattr(make_gen(), "gf", None) is not None:
            place(np.array([ce, np.float64(ce) / np.float64(q)], dtype=np.float64), A_EC)
        else:
            place(np.array([ce, (ce << 64) // q], dtype=np.uint64), A_EC)
        karg[16], karg[17], karg[18], karg[19], karg[20] = A_X, NF, A_P, NF, A_EC
        want = np.array([((int(a) - int(b)) * ce + int(c)) % q for a, b, c in zip(xe, want, pe)], dtype=np.uint64)
    place(karg, A_KARG)
    info = ""
    for blk in order:
        gen = make_gen()
        prog = gen.build()
        m = Machine(gen.T, 160 * 1024, mem.size)
        m.mem = mem
        m.vgpr[0] = np.arange(gen.T, dtype=np.uint32)
        m.vdef[0] = True
        m.sgpr[0], m.sgpr[1] = A_KARG, 0
        m.sgpr[gen.WGX.idx], m.sgpr[gen.WGY.idx], m.sgpr[4] = blk, 0, 0
        m.sdef[0:5] = True
        m.run(prog)
        mem = m.mem
        cnt = prog.count()
        info = "%d instructions, %d VALU" % (len(prog.ins), sum(n for op, n in cnt.items() if op.startswith("v_")))
    got = mem[A_OUT // 4: A_OUT // 4 + 2 * NF].view(np.uint64).copy()
    if fuse_last:
        assert not mem[A_FLAGS // 4: A_FLAGS // 4 + 0x400].any(), "the pair flags must be back at zero"
    elif inverse:
        # what ntt_top_kernel does next: last Gentleman-Sande stage and the scaling
        U = [int(a) for a in got[:N]]
        V = [int(a) for a in got[N:]]
        assert max(max(U), max(V)) < 8 * q
        w1n = psi[0]
        got = np.array([(u + v) * n_inv % q for u, v in zip(U, V)] + [(u - v) * w1n % q for u, v in zip(U, V)], dtype=np.uint64)
    ok = bool(np.array_equal(got, want))
    return ok, info


# A case is (label, [(key, run)], (word when good, word when bad)): key = (direction, mode, logn, threads, flavour), the arguments of
# catalogue.make and the catalogue key the part exercises; run(make_gen) -> (ok, info).  One line per case: every part must pass.
VERDICT = ("bit-exact vs oracle", "MISMATCH")
GROUPS = (2, 1, 1, 2, 3, 6)          # the digit-group addressing (grid z, skipped limbs)
ORDERS = ((0, 1), (1, 0))            # of a limb's two sub-block workgroups


def bits(q):
    return "q=%d (%d bits)" % (q, q.bit_length())


def run_cases(cases, list_only=False):
    """runs the cases and prints a line for each; list_only: prints the catalogue keys they exercise instead"""
    ok = True
    for label, parts, words in cases:
        good, info = True, None
        for (direction, mode, logn, threads, flavour), run in parts:
            if list_only:
                print(catalogue.key(direction, mode, logn, threads, **flavour))
                continue
            g, i = run(lambda: catalogue.make(direction, mode, logn, threads, **flavour))
            if info is None or not g:           # the first part's summary, or that of a part that failed
                info = i
            good = good and g
        ok = ok and good
        if not list_only:
            print("%s: %s; %s" % (label, words[not good], info), flush=True)
    return ok


def selftest_cases(logn, inverse=False, threads=1024):
    """every case on the seeded random input and on the stress polys of tests/limit_moduli.py (stress_inputs)"""
    d, head = ("inv", "inverse") if inverse else ("fwd", "forward")
    head += " logN=%d T=%d" % (logn, threads)
    key = lambda mode: (d, mode, logn, threads, {})

    def fams(q, geom=None, second=False):
        return lambda mk: over_families(logn, q, inverse, lambda x: emulate(mk(), inverse, q, geom, x=x), harshest_only=second)

    cases = []
    for mode in ((0, 1) if inverse else (0, 1, 2)):
        for q in test_moduli(logn, mode):
            # the last modulus of each mode also exercises the digit-group addressing
            geom = GROUPS if q == test_moduli(logn, mode)[-1] else None
            cases.append(("%s mode %d %s" % (head, mode, bits(q)), [(key(mode), fams(q, geom))], VERDICT))
    # grid x padded to a multiple of eight (lr_asm.cpp): the workgroups beyond n_items store nothing (integer kernels: x = limb)
    for mode in ((1,) if inverse else (1, 5)):
        pad = lambda mk: emulate(mk(), inverse, test_moduli(logn, 1)[0], (3, 1, 0, 0, 0, 4, 3))
        cases.append((head + " padding workgroup", [(key(mode), pad)], ("stores nothing", "WROTE")))
    for q in fp_test_moduli(logn):
        geom = GROUPS if q == fp_test_moduli(logn)[0] else None
        cases.append(("%s dual %s" % (head, bits(q)), [(key(3), fams(q, geom))], VERDICT))
    if not inverse:
        # the integer epilogue: the pure integer kernel of mode 1 ("m5") on the headline modulus and at both ends of its modulus range,
        # and the dual kernels' integer body on a modulus just above 2^46; then out = (x - NTT(in)) * c + plus on the FP64 body.
        # Each plain and with the digit-group addressing
        m1 = test_moduli(logn, 1)
        epilogues = [("integer epilogue", 5, q) for q in (m1[0], m1[1], m1[-1])] + [("integer epilogue", 4, fp_test_moduli(logn)[2])]
        epilogues += [("epilogue", 4, q) for q in fp_test_moduli(logn)[:2]]
        for name, mode, q in epilogues:
            for geom in (None, GROUPS):
                cases.append(("%s %s %s" % (head, name, bits(q)), [(key(mode), fams(q, geom, geom is not None))], VERDICT))
    return cases


def sub_cases(inverse=False):
    """the sub-block kernels of N = 2^16, on the seeded random input and the harshest stress polys"""
    d, head = ("inv", "inverse N=2^16 sub-blocks") if inverse else ("fwd", "forward N=2^16 sub-blocks")
    key = lambda mode, **flavour: (d, mode, 15, 1024, dict(flavour, sub=True))

    def fams(q, **kw):
        return lambda mk: over_families(16, q, inverse, lambda x: emulate_sub(mk, inverse, q, x=x, **kw))

    def variants(mode, q):
        if inverse:     # lazy outputs; the pair-flag kernels (last stage by whichever sub-block finishes second), both orders
            return [(key(mode), fams(q))] + [(key(mode, fuse_last=True), fams(q, order=order)) for order in ORDERS]
        # the top stage fused into the loads; the plain variant continues from the output of the separate top-stage pass
        return [(key(mode), fams(q)), (key(mode, fused=False), fams(q, pretop=True))]

    cases = []
    for mode in ((0, 1) if inverse else (0, 1, 2)):
        q = test_moduli(16, mode)[0]
        cases.append(("%s mode %d %s" % (head, mode, bits(q)), variants(mode, q), VERDICT))
    if not inverse:
        # the integer epilogue on the sub-block kernels: pure integer ("m5", fused top stage and plain), and the dual kernels' integer body
        for q in test_moduli(16, 1)[:2]:
            cases.append(("%s m5 fused-top %s" % (head, bits(q)), [(key(5), fams(q, pretop=False))], VERDICT))
            cases.append(("%s m5 plain %s" % (head, bits(q)), [(key(5, fused=False), fams(q, pretop=True))], VERDICT))
        q = fp_test_moduli(16)[2]
        cases.append(("%s dual integer-body epilogue %s" % (head, bits(q)), [(key(4, fused=False), fams(q, pretop=True))], VERDICT))
    for q in fp_test_moduli(16)[:2]:
        parts = variants(3, q) + ([] if inverse else [(key(4, fused=False), fams(q, pretop=True))])
        cases.append(("%s dual %s" % (head, bits(q)), parts, VERDICT))
    if not inverse:
        # the epilogue behind the fused top stage (lr_ntt_fwd16s_m4, route Fwd16Fused with an epilogue): FP64 body and integer body
        for q in (fp_test_moduli(16)[0], fp_test_moduli(16)[2]):
            cases.append(("%s dual fused-top epilogue %s" % (head, bits(q)), [(key(4), fams(q, pretop=False))], VERDICT))
    return cases


def halves_cases(inverse=False):
    """N = 2^15 as two 2^14 sub-blocks (small launches: twice the workgroups, half the latency): the plain forward sub-block kernels
    ("h": the stage over bit 14 applied before, by the basis extension or ntt_top_kernel) in every mode incl. the epilogues, the lazy inverse
    ones; on the seeded random input and the harshest stress polys, the integer modes at the top of their modulus range; both orders"""
    d, head = ("inv", "inverse N=2^15 halves") if inverse else ("fwd", "forward N=2^15 halves")
    cases = [("mode %d" % mode, mode, test_moduli(15, mode)[0]) for mode in ((0, 1) if inverse else (0, 1, 2))]
    cases.append(("mode 1", 1, test_moduli(15, 1)[1]))
    if not inverse:
        cases.append(("m5", 5, test_moduli(15, 1)[0]))
    for q in fp_test_moduli(15):
        cases += [("dual", 3, q)] + ([] if inverse else [("dual epilogue", 4, q)])
    out = []
    for name, mode, q in cases:
        runs = [lambda mk, q=q, order=order: over_families(15, q, inverse, lambda x: emulate_sub(mk, inverse, q, pretop=not inverse, order=order, x=x))
                for order in ORDERS]
        key = (d, mode, 14, 1024, {"sub": True} if inverse else {"sub": True, "fused": False})
        out.append(("%s %s %s" % (head, name, bits(q)), [(key, run) for run in runs], VERDICT))
    return out


def main(argv):
    list_only = "--list-cases" in argv
    argv = [a for a in argv if a != "--list-cases"]
    logn = int(argv[0])
    inverse = argv[1:2] == ["--selftest-inverse"]
    if argv[-1] == "--halves":
        cases = halves_cases(inverse)
    elif logn == 16:
        cases = sub_cases(inverse)
    elif argv[1:2] == ["--selftest-persist"]:
        cases = persist_cases()
    else:
        cases = selftest_cases(logn, inverse, int(argv[2]) if len(argv) > 2 else 1024)
    return run_cases(cases, list_only)


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1:]) else 1)
