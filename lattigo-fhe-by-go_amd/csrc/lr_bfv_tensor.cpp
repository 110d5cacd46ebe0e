// lr_bfv_tensor.cpp -- C ABI: bfv.Evaluator.Mul for operands that are not both of degree 1 (tensorAndRescale, bfv/evaluator.go:371-415).
//
// A translation unit of its own, outside the lr_abi_* family: it is the one caller of launch_tensor_deg.
#include "lr_host.hpp"

// ------------------------------------------------------------------------------------------
// bfv.Evaluator.Mul (:467) -> tensorAndRescale (:278-464) for every degree pair with d0 + d1 <= 5
// ------------------------------------------------------------------------------------------
extern "C" int lr_bfv_mul_deg(lr_bfv_plan *pl, const lr_poly *const *ct0, int deg0, const lr_poly *const *ct1, int deg1,
                              lr_poly *const *out) {
    return guarded([&]() -> int {
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
    // the degree-1 x degree-1 branch (:320-369) is other code: lr_bfv_mul, the same bits by construction
    if (deg0 == 1 && deg1 == 1) return lr_bfv_mul(pl, ct0[0], ct0[1], ct1[0], ct1[1], out[0], out[1], out[2]);
    lr_context *cQ = pl->cQ, *cM = pl->cM;
    const int nQ = cQ->h.L(), nM = cM->h.L(), n = (int)cQ->h.N;
    const int batch = ct0[0]->batch;
    if (batch > pl->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the plan's max_batch");
    auto shape_ok = [&](const lr_poly *p) { return p->N == cQ->h.N && p->limbs >= nQ && p->batch == batch; };
    for (int i = 0; i < nA; ++i)
        if (!shape_ok(ct0[i])) return fail(LR_ERR_SHAPE, "BFV Mul: operands must hold |Q| limbs and share the batch");
    for (int j = 0; j < nB; ++j)
        if (!shape_ok(ct1[j])) return fail(LR_ERR_SHAPE, "BFV Mul: operands must hold |Q| limbs and share the batch");
    for (int k = 0; k < nout; ++k)
        if (!shape_ok(out[k])) return fail(LR_ERR_SHAPE, "BFV Mul: operands must hold |Q| limbs and share the batch");
    LR_TRY(same_stream(cQ, cM));
    LR_HIP(hipSetDevice(cQ->device));
    // ct0 == ct1 (Go's pointer comparison, :306 and :379): the same handles in the same order.  The operand is lifted once; in the reachable
    // domain that is 2 x 2 (degree 3 squared needs c[6]).
    bool square = deg0 == deg1;
    for (int i = 0; square && i < nA; ++i) square = ct0[i] == ct1[i];
    const int nin = square ? nA : nA + nB;        // operand polys lifted: slots 0..nA-1 = ct0, then ct1
    const long long sQ = (long long)nQ * n, sM = (long long)nM * n;
    const long long slotQ = (long long)batch * sQ, slotM = (long long)batch * sM;
    LR_TRY(pl->liftQ.ensure(cQ, (size_t)nin * batch * sQ));
    LR_TRY(pl->liftM.ensure(cQ, (size_t)nin * batch * sM));
    LR_TRY(pl->prodQ.ensure(cQ, (size_t)nout * batch * sQ));
    LR_TRY(pl->prodM.ensure(cQ, (size_t)nout * batch * sM));
    const lr_poly *src[2 * (kTensorMaxDegree + 1)];
    for (int i = 0; i < nA; ++i) src[i] = ct0[i];
    for (int j = 0; !square && j < nB; ++j) src[nA + j] = ct1[j];
    lr_bext *bx = pl->bext;
    // :298-313 for every operand poly, before any output is written (so an output may be an operand).  A small batch is gathered into one
    // batch of nin B and lifted in one pass, as lr_bfv_mul gathers its four; the threshold counts the polys lifted.
    const bool gathered = !pl->no_gather && (long long)nin * batch * std::max(nQ, nM) * (n >= (1 << 15) ? 2 : 1) <= pl->gather_below;
    if (gathered) {
        LR_TRY(pl->stageIn.ensure(cQ, (size_t)nin * batch * sQ));
        LR_TRY(pl->stageOut.ensure(cQ, (size_t)nout * batch * sQ));
        MultiCopyLaunch G{};
        for (int k = 0; k < nin; ++k) {
            G.src[k] = src[k]->d;
            G.src_stride[k] = src[k]->stride();
            G.dst[k] = pl->stageIn.d + k * slotQ;
            G.dst_stride[k] = sQ;
        }
        G.count = nin;
        G.batch = batch;
        G.n = n;
        LR_HIP(launch_multicopy(G, nQ, cQ->stream));
        Rows in{pl->stageIn.d, sQ, 0, 1};
        LR_TRY(run_ext(cQ, bx->qp, nQ, in, nin * batch, segment(pl->liftM.d, sM, 0, 0, nM), segment(nullptr, 0, 0, 0, 0)));
        LR_TRY(run_ntt(cQ, false, in, Rows{pl->liftQ.d, sQ, 0, 1}, 0, 1, nQ, nin * batch));
        LR_TRY(run_ntt(cM, false, Rows{pl->liftM.d, sM, 0, 1}, Rows{pl->liftM.d, sM, 0, 1}, 0, 1, nM, nin * batch));
    } else {
        for (int k = 0; k < nin; ++k) {
            u64 *dQ = pl->liftQ.d + k * slotQ, *dM = pl->liftM.d + k * slotM;
            LR_TRY(run_ext(cQ, bx->qp, nQ, rows_of(src[k]), batch, segment(dM, sM, 0, 0, nM), segment(nullptr, 0, 0, 0, 0)));
            LR_TRY(run_ntt(cQ, false, rows_of(src[k]), Rows{dQ, sQ, 0, 1}, 0, 1, nQ, batch));
            LR_TRY(run_ntt(cM, false, Rows{dM, sM, 0, 1}, Rows{dM, sM, 0, 1}, 0, 1, nM, batch));
        }
    }
    // :371-415 the tensor, one pass per base: the accumulators are zeroed, MForm'd and summed in registers (every one canonical)
    for (int base = 0; base < 2; ++base) {
        lr_context *cx = base == 0 ? cQ : cM;
        u64 *lift = base == 0 ? pl->liftQ.d : pl->liftM.d, *prod = base == 0 ? pl->prodQ.d : pl->prodM.d;
        const long long slot = base == 0 ? slotQ : slotM;
        TensorDegLaunch T{};
        for (int i = 0; i < nA; ++i) T.a[i] = lift + i * slot;
        for (int j = 0; j < nB; ++j) T.b[j] = square ? T.a[j] : lift + (nA + j) * slot;
        for (int k = 0; k < nout; ++k) T.c[k] = prod + k * slot;
        T.stride = base == 0 ? sQ : sM;
        T.n = n;
        T.lp = cx->d_lp;
        LR_HIP(launch_tensor_deg(T, deg0, deg1, square, base == 0 ? nQ : nM, batch, cx->stream));
    }
    // :417-463 for every output component: the tail of lr_bfv_mul (back to coefficients, divide by Q, centre, back to Q, times t)
    const bool fuse_down = !pl->no_ext_epilogue && ext_epilogue_supported(bx->qp.tables(), nQ, n);
    const bool fuse_up = !pl->no_ext_epilogue && ext_epilogue_supported(bx->pq.tables(), nM, n);
    const int rounds = gathered ? 1 : nout, nb = gathered ? nout * batch : batch;
    if (!fuse_down) LR_TRY(bx->poolP.ensure(cM, (size_t)nb * sM));
    for (int i = 0; i < rounds; ++i) {
        u64 *const cq = pl->prodQ.d + i * slotQ, *const cm = pl->prodM.d + i * slotM;
        u64 *const outp = gathered ? pl->stageOut.d : out[i]->d;
        const long long outs = gathered ? sQ : out[i]->stride();
        Rows q1{cq, sQ, 0, 1}, q2{cm, sM, 0, 1};
        LR_TRY(run_ntt(cQ, true, q1, q1, 0, 1, nQ, nb));
        LR_TRY(run_ntt(cM, true, q2, q2, 0, 1, nM, nb));
        // ModDownSplitedQP (:450) with the AddScalarBigint(pHalf) of :457
        if (fuse_down) {
            ExtSegment sd = segment(cm, sM, 0, 0, nM);
            sd.epi_mode = 1;
            sd.epi_x = cm;
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
    if (gathered) {
        MultiCopyLaunch S{};
        for (int k = 0; k < nout; ++k) {
            S.src[k] = pl->stageOut.d + k * slotQ;
            S.src_stride[k] = sQ;
            S.dst[k] = out[k]->d;
            S.dst_stride[k] = out[k]->stride();
        }
        S.count = nout;
        S.batch = batch;
        S.n = n;
        LR_HIP(launch_multicopy(S, nQ, cQ->stream));
    }
    return LR_OK;
    });
}
