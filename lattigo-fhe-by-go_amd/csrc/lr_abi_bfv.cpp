// lr_abi_bfv.cpp -- C ABI: lr_bfv_plan and bfv.Evaluator.Mul (tensorAndRescale): lr_bfv_mul and lr_bfv_mul_deg, two entry points of one pipeline.
#include "lr_host.hpp"

// ------------------------------------------------------------------------------------------
// lr_bfv_plan: what bfv.NewEvaluator builds for Mul (bfv/evaluator.go:89-112)
// ------------------------------------------------------------------------------------------
namespace lr_host {
// (prod of moduli) >> 1, then reduced modulo every prime of `targets` (little-endian multi-precision)
void half_product_residues(const std::vector<u64> &moduli, const std::vector<u64> &targets, LimbScalars &out) {
    std::vector<u64> big(1, 1);
    for (u64 m : moduli) {
        u64 carry = 0;
        for (size_t i = 0; i < big.size(); ++i) {
            const u128 p = (u128)big[i] * m + carry;
            big[i] = (u64)p;
            carry = (u64)(p >> 64);
        }
        if (carry) big.push_back(carry);
    }
    for (size_t i = 0; i < big.size(); ++i) big[i] = (big[i] >> 1) | (i + 1 < big.size() ? (big[i + 1] << 63) : 0);
    std::memset(&out, 0, sizeof(out));
    for (size_t k = 0; k < targets.size(); ++k) {
        u64 r = 0;
        for (size_t i = big.size(); i-- > 0;) r = (u64)((((u128)r << 64) | big[i]) % targets[k]);
        out.v[k] = r;
    }
}
}  // namespace lr_host

extern "C" int lr_bfv_plan_create(lr_context *cQ, lr_context *cM, uint64_t t, int max_batch, lr_bfv_plan **out) {
    return lr_bfv_plan_create_ex(cQ, cM, t, max_batch, nullptr, out);
}

extern "C" int lr_bfv_plan_create_ex(lr_context *cQ, lr_context *cM, uint64_t t, int max_batch, const lr_options *options, lr_bfv_plan **out) {
    return guarded([&]() -> int {
    if (!cQ || !cM || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    Options parsed = cQ->opt;                                   // options == NULL: the options of ctxQ, as the header says
    if (options) LR_TRY(options_from_public(options, &parsed));
    else parsed.apply_env();
    if (max_batch < 1) return fail(LR_ERR_ARG, "max_batch must be >= 1");
    LR_TRY(same_degree(cQ, cM));
    std::unique_ptr<lr_bfv_plan> p(new lr_bfv_plan());
    p->cQ = cQ;
    p->cM = cM;
    p->device = cQ->device;
    p->t = t;
    p->max_batch = max_batch;
    half_product_residues(cM->h.q, cQ->h.q, p->phalf_q);
    half_product_residues(cM->h.q, cM->h.q, p->phalf_m);
    std::memset(&p->t_mont, 0, sizeof(p->t_mont));
    for (int i = 0; i < cQ->h.L(); ++i)
        p->t_mont.v[i] = mform(bred_add(t, cQ->h.q[i], cQ->h.bred[i].hi), cQ->h.q[i], cQ->h.bred[i].hi, cQ->h.bred[i].lo);
    LR_HIP(hipSetDevice(cQ->device));
    LR_TRY(to_device(&p->d_phalf_q, p->phalf_q.v, (size_t)cQ->h.L()));
    LR_TRY(to_device(&p->d_phalf_m, p->phalf_m.v, (size_t)cM->h.L()));
    LR_TRY(to_device(&p->d_t_mont, p->t_mont.v, (size_t)cQ->h.L()));
    p->no_ext_epilogue = parsed.bfv_no_ext_epilogue;
    p->no_gather = parsed.bfv_no_gather;
    p->gather_below = parsed.bfv_gather_below;
    LR_TRY(lr_bext_create(cQ, cM, &p->bext));
    *out = p.release();
    return LR_OK;
    });
}

extern "C" int lr_bfv_plan_destroy(lr_bfv_plan *p) {
    return guarded([&]() -> int {
    if (!p) return LR_OK;
    if (p->lane_of) return fail(LR_ERR_ARG, "this plan is a lane of a live batcher: destroy the batcher first");
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its contexts' caller-supplied stream
    lr_bext_destroy(p->bext);
    delete p;
    return LR_OK;
    });
}

// ------------------------------------------------------------------------------------------
// bfv.Evaluator.Mul (:467) -> tensorAndRescale (:278-464) for every degree pair with 1 <= d0 + d1 <= 5: ONE host pipeline in three
// stages (lift, tensor, rescale tail) behind the two entry points lr_bfv_mul (degree 1 x degree 1, fixed arity) and lr_bfv_mul_deg.
// ------------------------------------------------------------------------------------------
namespace lr_host {
namespace {
// the derived sizes of one call
struct BfvMulShape {
    int deg0, deg1, nA, nB, nout;
    bool square;             // ct0 == ct1: the operand is lifted once and the tensor reads its slots twice
    int nin;                 // operand polys lifted: slots 0..nA-1 = ct0, then ct1 (for 1 x 1: a0, a1, b0, b1)
    bool gathered;           // a small batch: the operands are lifted as one batch of nin B, the products go down as one of nout B
    int nQ, nM, n, batch;
    long long sQ, sM;        // poly strides of the pools over Q and over QMul
    long long slotQ, slotM;  // batch * stride: one slot
};

// null handles, the degree domain, distinct outputs, N / limbs / batch of every poly, batch <= max_batch
int bfv_mul_check(const lr_bfv_plan *pl, const lr_poly *const *ct0, int deg0, const lr_poly *const *ct1, int deg1, lr_poly *const *out) {
    if (!pl || !ct0 || !ct1 || !out) return fail(LR_ERR_ARG, "null argument");
    // bfv.NewEvaluator's pools hold 6 polys (:74-82): a larger product is an index panic in Go, degree 0 x 0 one of
    // getElemAndCheckBinary (:114)
    if (deg0 < 0 || deg1 < 0 || deg0 + deg1 < 1 || deg0 + deg1 > kTensorMaxDegree)
        return fail(LR_ERR_ARG, "BFV Mul: the operand degrees must satisfy deg0, deg1 >= 0 and 1 <= deg0 + deg1 <= 5");
    const int nA = deg0 + 1, nB = deg1 + 1, nout = deg0 + deg1 + 1;
    for (int i = 0; i < nA; ++i)
        if (!ct0[i]) return fail(LR_ERR_ARG, "null argument");
    for (int j = 0; j < nB; ++j)
        if (!ct1[j]) return fail(LR_ERR_ARG, "null argument");
    for (int k = 0; k < nout; ++k) {
        if (!out[k]) return fail(LR_ERR_ARG, "null argument");
        for (int l = 0; l < k; ++l)
            if (out[l] == out[k]) return fail(LR_ERR_ARG, "BFV Mul: the output polys must be distinct");
    }
    const lr_context *cQ = pl->cQ;
    const int nQ = cQ->h.L(), batch = ct0[0]->batch;
    if (batch > pl->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the plan's max_batch");
    for (int i = 0; i < nA + nB + nout; ++i) {
        const lr_poly *p = i < nA ? ct0[i] : i < nA + nB ? ct1[i - nA] : out[i - nA - nB];
        if (p->N != cQ->h.N || p->limbs < nQ || p->batch != batch) return fail(LR_ERR_SHAPE, "BFV Mul: operands must hold |Q| limbs and share the batch");
    }
    return LR_OK;
}

// :298-313 basis extension Q -> QMul, then NTT in both bases, for every operand poly src[0..nin-1] into its slot of liftQ / liftM
int bfv_lift(lr_bfv_plan *pl, const BfvMulShape &s, const lr_poly *const *src) {
    lr_context *cQ = pl->cQ, *cM = pl->cM;
    lr_bext *bx = pl->bext;
    const int nQ = s.nQ, nM = s.nM;
    const long long sQ = s.sQ, sM = s.sM;
    if (s.gathered) {
        // the operand polys (unrelated addresses) are gathered into one batch of nin B and every step runs once on it.  One ciphertext pair
        // at PN14QP438: 26 launches of 3 - 6 workgroups in a row, 424 us; 11 launches, 138 us (profiles/r03/bfv_small_batch.txt).  The
        // copies buy nothing once a launch of one operand fills the chip.
        LR_TRY(pl->stageIn.ensure(cQ, (size_t)s.nin * s.batch * sQ));
        MultiCopyLaunch G{};
        for (int k = 0; k < s.nin; ++k) {
            G.src[k] = src[k]->d;
            G.src_stride[k] = src[k]->stride();
            G.dst[k] = pl->stageIn.d + k * s.slotQ;
            G.dst_stride[k] = sQ;
        }
        G.count = s.nin;
        G.batch = s.batch;
        G.n = s.n;
        LR_HIP(launch_multicopy(G, nQ, cQ->stream));
        Rows in{pl->stageIn.d, sQ, 0, 1};
        LR_TRY(run_ext(cQ, bx->qp, nQ, in, s.nin * s.batch, segment(pl->liftM.d, sM, 0, 0, nM), segment(nullptr, 0, 0, 0, 0)));
        LR_TRY(run_ntt(cQ, false, in, Rows{pl->liftQ.d, sQ, 0, 1}, 0, 1, nQ, s.nin * s.batch));
        LR_TRY(run_ntt(cM, false, Rows{pl->liftM.d, sM, 0, 1}, Rows{pl->liftM.d, sM, 0, 1}, 0, 1, nM, s.nin * s.batch));
        return LR_OK;
    }
    for (int k = 0; k < s.nin; ++k) {
        u64 *dQ = pl->liftQ.d + k * s.slotQ, *dM = pl->liftM.d + k * s.slotM;
        LR_TRY(run_ext(cQ, bx->qp, nQ, rows_of(src[k]), s.batch, segment(dM, sM, 0, 0, nM), segment(nullptr, 0, 0, 0, 0)));
        LR_TRY(run_ntt(cQ, false, rows_of(src[k]), Rows{dQ, sQ, 0, 1}, 0, 1, nQ, s.batch));
        LR_TRY(run_ntt(cM, false, Rows{dM, sM, 0, 1}, Rows{dM, sM, 0, 1}, 0, 1, nM, s.batch));
    }
    return LR_OK;
}

// the tensor, one pass per base, from the lift slots into product slots 0..nout-1.  The one stage that tells 1 x 1 from the rest:
//   1 x 1 (:320-369): MForm x2 and the four products, the kernel ckks MulRelin shares (the middle component comes out reduced where the
//     reference leaves it in [0,2q): the InvNTT that follows is canonical either way).  Squaring (:306, :334) is b0 == a0: its tensor
//     (c0 = a0^2, c1 = 2 a0 a1 by AddNoMod, c2 = a1^2) and the regular one give the same canonical polys after the InvNTT -- MRed(MForm(x), y)
//     and MRed(MForm(y), x) are the same residue below q --, so the kernel simply reads the first operand's slots twice;
//   every other pair (:371-415): the accumulators are zeroed, MForm'd and summed in registers (every one canonical).
int bfv_tensor(lr_bfv_plan *pl, const BfvMulShape &s) {
    for (int base = 0; base < 2; ++base) {
        lr_context *cx = base == 0 ? pl->cQ : pl->cM;
        u64 *lift = base == 0 ? pl->liftQ.d : pl->liftM.d, *prod = base == 0 ? pl->prodQ.d : pl->prodM.d;
        const long long slot = base == 0 ? s.slotQ : s.slotM, stride = base == 0 ? s.sQ : s.sM;
        const int limbs = base == 0 ? s.nQ : s.nM;
        if (s.deg0 == 1 && s.deg1 == 1) {
            TensorLaunch T;
            T.a0 = lift;
            T.a1 = lift + slot;
            T.b0 = s.square ? T.a0 : lift + 2 * slot;
            T.b1 = s.square ? T.a1 : lift + 3 * slot;
            T.a0_stride = T.a1_stride = T.b0_stride = T.b1_stride = stride;
            T.c0 = prod;
            T.c1 = prod + slot;
            T.c2 = prod + 2 * slot;
            T.c_stride = T.c1_stride = T.c2_stride = stride;
            T.n = s.n;
            T.lp = cx->d_lp;
            LR_HIP(launch_tensor(T, limbs, s.batch, cx->stream));
        } else {
            TensorDegLaunch T{};
            for (int i = 0; i < s.nA; ++i) T.a[i] = lift + i * slot;
            for (int j = 0; j < s.nB; ++j) T.b[j] = s.square ? T.a[j] : lift + (s.nA + j) * slot;
            for (int k = 0; k < s.nout; ++k) T.c[k] = prod + k * slot;
            T.stride = stride;
            T.n = s.n;
            T.lp = cx->d_lp;
            LR_HIP(launch_tensor_deg(T, s.deg0, s.deg1, s.square, limbs, s.batch, cx->stream));
        }
    }
    return LR_OK;
}

// :417-463 for every product: back to coefficients, divide by Q (result over QMul), centre, back to Q, times t -- into the callers' polys,
// one product after the other, or (gathered) as one batch of nout B whose results are scattered afterwards
int bfv_rescale(lr_bfv_plan *pl, const BfvMulShape &s, lr_poly *const *out) {
    lr_context *cQ = pl->cQ, *cM = pl->cM;
    lr_bext *bx = pl->bext;
    const int nQ = s.nQ, nM = s.nM, n = s.n;
    const long long sQ = s.sQ, sM = s.sM;
    // the element-wise tails ride in the extensions' stores where the extension kernel in use has the epilogue (ExtSegment::epi_mode)
    const bool fuse_down = !pl->no_ext_epilogue && ext_epilogue_supported(bx->qp.tables(), nQ, n);
    const bool fuse_up = !pl->no_ext_epilogue && ext_epilogue_supported(bx->pq.tables(), nM, n);
    const int rounds = s.gathered ? 1 : s.nout, nb = s.gathered ? s.nout * s.batch : s.batch;
    if (s.gathered) LR_TRY(pl->stageOut.ensure(cQ, (size_t)s.nout * s.batch * sQ));
    if (!fuse_down) LR_TRY(bx->poolP.ensure(cM, (size_t)nb * sM));
    for (int i = 0; i < rounds; ++i) {
        u64 *const cq = pl->prodQ.d + i * s.slotQ, *const cm = pl->prodM.d + i * s.slotM;
        u64 *const outp = s.gathered ? pl->stageOut.d : out[i]->d;
        const long long outs = s.gathered ? sQ : out[i]->stride();
        Rows q1{cq, sQ, 0, 1}, q2{cm, sM, 0, 1};
        LR_TRY(run_ntt(cQ, true, q1, q1, 0, 1, nQ, nb));
        LR_TRY(run_ntt(cM, true, q2, q2, 0, 1, nM, nb));
        // ModDownSplitedQP(levelQ, levelQMul, c2Q1, c2Q2, c2Q2), ring_basis_extension.go:314, with the AddScalarBigint(pHalf) of :457
        if (fuse_down) {
            ExtSegment sd = segment(cm, sM, 0, 0, nM);
            sd.epi_mode = 1;
            sd.epi_x = cm;                         // read and written at the same position by the same thread
            sd.epi_x_stride = sM;
            sd.epi_c = bx->d_moddown_qp;
            sd.epi_s = pl->d_phalf_m;
            LR_TRY(run_ext(cQ, bx->qp, nQ, q1, nb, sd, segment(nullptr, 0, 0, 0, 0)));
        } else {
            LR_TRY(run_ext(cQ, bx->qp, nQ, q1, nb, segment(bx->poolP.d, sM, 0, 0, nM), segment(nullptr, 0, 0, 0, 0)));
            LR_TRY(run_submul(cM, nM, nb, cm, sM, bx->poolP.d, sM, (long long)n, cm, sM, bx->d_moddown_qp, false, nullptr, nullptr, 0,
                              &pl->phalf_m));
        }
        // :458 ModUpSplitPQ, :459 SubScalarBigint(pHalf), :462 MulScalar(t)
        if (fuse_up) {
            ExtSegment su = segment(outp, outs, 0, 0, nQ);
            su.epi_mode = 2;
            su.epi_c = pl->d_t_mont;
            su.epi_s = pl->d_phalf_q;
            LR_TRY(run_ext(cQ, bx->pq, nM, q2, nb, su, segment(nullptr, 0, 0, 0, 0)));
        } else {
            LR_TRY(run_ext(cQ, bx->pq, nM, q2, nb, segment(outp, outs, 0, 0, nQ), segment(nullptr, 0, 0, 0, 0)));
            ScalarPairLaunch S;
            S.in = outp;
            S.out = outp;
            S.in_stride = S.out_stride = outs;
            S.n = n;
            S.lp = cQ->d_lp;
            S.sub = pl->phalf_q;
            S.mul = pl->t_mont;
            LR_HIP(launch_scalar_pair(S, nQ, nb, cQ->stream));
        }
    }
    if (s.gathered) {
        MultiCopyLaunch S{};
        for (int k = 0; k < s.nout; ++k) {
            S.src[k] = pl->stageOut.d + k * s.slotQ;
            S.src_stride[k] = sQ;
            S.dst[k] = out[k]->d;
            S.dst_stride[k] = out[k]->stride();
        }
        S.count = s.nout;
        S.batch = s.batch;
        S.n = n;
        LR_HIP(launch_multicopy(S, nQ, cQ->stream));
    }
    return LR_OK;
}

// the arguments have passed bfv_mul_check
int bfv_tensor_and_rescale(lr_bfv_plan *pl, const lr_poly *const *ct0, int deg0, const lr_poly *const *ct1, int deg1, lr_poly *const *out) {
    lr_context *cQ = pl->cQ, *cM = pl->cM;
    LR_TRY(same_stream(cQ, cM));
    LR_HIP(hipSetDevice(cQ->device));
    BfvMulShape s;
    s.deg0 = deg0, s.deg1 = deg1;
    s.nA = deg0 + 1, s.nB = deg1 + 1, s.nout = deg0 + deg1 + 1;
    // ct0 == ct1 (Go's pointer comparison, :306 and :379): the same handles in the same order.  The operand is lifted once; in the reachable
    // domain that is 1 x 1 and 2 x 2 (degree 3 squared needs c[6]).
    s.square = deg0 == deg1;
    for (int i = 0; s.square && i < s.nA; ++i) s.square = ct0[i] == ct1[i];
    s.nin = s.square ? s.nA : s.nA + s.nB;
    s.nQ = cQ->h.L(), s.nM = cM->h.L(), s.n = (int)cQ->h.N, s.batch = ct0[0]->batch;
    s.sQ = (long long)s.nQ * s.n, s.sM = (long long)s.nM * s.n;
    s.slotQ = s.batch * s.sQ, s.slotM = s.batch * s.sM;
    // workgroups of the operands' joint transform up to which they are gathered: the polys lifted.  1 x 1 counts its four
    // operand polys even when squaring, where two are lifted -- the threshold it was measured with; no 1 x 1 call changes path.
    const int counted = deg0 == 1 && deg1 == 1 ? s.nA + s.nB : s.nin;
    s.gathered = !pl->no_gather && (long long)counted * s.batch * std::max(s.nQ, s.nM) * (s.n >= (1 << 15) ? 2 : 1) <= pl->gather_below;
    LR_TRY(pl->liftQ.ensure(cQ, (size_t)s.nin * s.batch * s.sQ));
    LR_TRY(pl->liftM.ensure(cQ, (size_t)s.nin * s.batch * s.sM));
    LR_TRY(pl->prodQ.ensure(cQ, (size_t)s.nout * s.batch * s.sQ));
    LR_TRY(pl->prodM.ensure(cQ, (size_t)s.nout * s.batch * s.sM));
    const lr_poly *src[2 * (kTensorMaxDegree + 1)];
    for (int i = 0; i < s.nA; ++i) src[i] = ct0[i];
    for (int j = 0; !s.square && j < s.nB; ++j) src[s.nA + j] = ct1[j];
    // every operand is lifted before any output is written, so an output may be an operand
    LR_TRY(bfv_lift(pl, s, src));
    LR_TRY(bfv_tensor(pl, s));
    return bfv_rescale(pl, s, out);
}
}  // namespace
}  // namespace lr_host

extern "C" int lr_bfv_mul(lr_bfv_plan *pl, const lr_poly *a0, const lr_poly *a1, const lr_poly *b0, const lr_poly *b1,
                          lr_poly *o0, lr_poly *o1, lr_poly *o2) {
    return guarded([&]() -> int {
    const lr_poly *const ct0[2] = {a0, a1}, *const ct1[2] = {b0, b1};
    lr_poly *const out[3] = {o0, o1, o2};
    LR_TRY(bfv_mul_check(pl, ct0, 1, ct1, 1, out));
    return bfv_tensor_and_rescale(pl, ct0, 1, ct1, 1, out);
    });
}

extern "C" int lr_bfv_mul_deg(lr_bfv_plan *pl, const lr_poly *const *ct0, int deg0, const lr_poly *const *ct1, int deg1,
                              lr_poly *const *out) {
    return guarded([&]() -> int {
    LR_TRY(bfv_mul_check(pl, ct0, deg0, ct1, deg1, out));
    return bfv_tensor_and_rescale(pl, ct0, deg0, ct1, deg1, out);
    });
}
