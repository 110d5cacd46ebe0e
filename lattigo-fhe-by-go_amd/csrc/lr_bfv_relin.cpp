// lr_bfv_relin.cpp -- C ABI: bfv.evaluator.Relinearize of every degree as one call on an lr_ckks_plan, lr_bfv_relinearize_deg
// (bfv/evaluator.go:480-499, 509-522):
//   (a0, a1) = (ct[0], ct[1]);   for deg = degree .. 2:  (p0, p1) = switchKeys(ct[deg], evakey[deg - 2]);  a0 = CRed(a0 + p0);  a1 = CRed(a1 + p1)
// The degree - 1 key switches share no data.  The composed route runs them one after the other as lr_bfv_relinearize does
// (bfv_switch_keys_core, LR_ADD x2).  The merged route runs G of them as ONE key switch over G * batch members with one key per group
// (bfv_switch_keys_grouped, lr_abi_ckks.cpp) and adds the pass's G results to the running pair in one launch (launch_bfv_relin_fold,
// lr_ewise.hip), in the reference's order.  Same bits on both.
// The unit's name keeps it out of the lr_abi_*.cpp set (its launcher has a stand-in of its own under tests/cpp).
#include "lr_host.hpp"

namespace lr_host {
namespace {

enum class RelinRoute { Merged, Composed };
// THE route decision of a relinearisation: merged passes of G degrees, unless the plan or its context asks for the
// call-by-call shape (lr_options::no_epilogue, as the rotation chains read it).  Measured on one MI355X against the composed route with the
// same key-switch kernels, in the same run (a plan with max_batch 256): the merged route wins wherever G >= 2 -- PN14QP438
// degree 5, one ciphertext 148 us against 457 us, 64 ciphertexts 1621 against 1782; PN13QP218 degree 3, one ciphertext 105 against 182 --
// and with G = 1 (the batch fills max_batch: per degree the same key switch, then one fold instead of two Adds) the two are within the
// spread of the repeated medians at every size measured (PN14QP438 degree 5 at 256: 6432 against 6397 us, spread 80).  No regime goes to
// the composed route on speed.
RelinRoute relin_route(const lr_ckks_plan *pl) {
    if (pl->opt.no_epilogue || pl->cQ->opt.no_epilogue) return RelinRoute::Composed;
    return RelinRoute::Merged;
}

// the running pair: the caller's polys
struct Comp {
    u64 *d;
    long long stride;
};

// :494-495 as lr_bfv_relinearize launches them: one ciphertext's two additions as one launch where the operands allow it
int add_pair(lr_ckks_plan *pl, int batch, const Comp (&a)[2], const u64 *p0, const u64 *p1, long long p_stride, const Comp (&out)[2]) {
    lr_context *cQ = pl->cQ;
    const int L1 = cQ->h.L();
    const ComponentPair ins = component_pair(a[0].d, a[0].stride, a[1].d, a[1].stride, batch);
    const ComponentPair outs = component_pair(out[0].d, out[0].stride, out[1].d, out[1].stride, batch);
    if (batch == 1 && !pl->opt.no_pair && ins && outs && p1 == p0 + p_stride)
        return run_ewise(cQ, LR_ADD, L1, 2, a[0].d, ins.stride, p0, p_stride, out[0].d, outs.stride, nullptr);
    LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, a[0].d, a[0].stride, p0, p_stride, out[0].d, out[0].stride, nullptr));      // :494
    return run_ewise(cQ, LR_ADD, L1, batch, a[1].d, a[1].stride, p1, p_stride, out[1].d, out[1].stride, nullptr);       // :495
}

// the relinearisation itself; every argument checked
int relin_core(lr_ckks_plan *pl, const lr_poly *const *ct, int degree, const lr_poly *const *evks, lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = pl->cQ;
    const int batch = ct[0]->batch, L1 = cQ->h.L(), n = (int)cQ->h.N;
    const long long s = (long long)L1 * n;
    LR_TRY(same_stream(pl->cQ, pl->cP));
    LR_HIP(hipSetDevice(pl->device));
    Comp a[2] = {{ct[0]->d, ct[0]->stride()}, {ct[1]->d, ct[1]->stride()}};
    const Comp out[2] = {{o0->d, o0->stride()}, {o1->d, o1->stride()}};
    if (degree == 1) {
        for (int k = 0; k < 2; ++k)
            if (a[k].d != out[k].d) LR_TRY(run_ewise(cQ, LR_COPY, L1, batch, a[k].d, a[k].stride, nullptr, 0, out[k].d, out[k].stride, nullptr));
        return LR_OK;
    }
    if (relin_route(pl) == RelinRoute::Composed) {
        LR_TRY(pl->bfvP.ensure(cQ, (size_t)2 * batch * s));         // keyswitchpool[2], [3] (:489-490)
        u64 *const p0 = pl->bfvP.d, *const p1 = pl->bfvP.d + (long long)batch * s;
        for (int deg = degree; deg > 1; --deg) {
            LR_TRY(bfv_switch_keys_core(pl, batch, ct[deg]->d, ct[deg]->stride(), evks[deg - 2], {{p0, p1}, {s, s}}));     // :493
            LR_TRY(add_pair(pl, batch, a, p0, p1, s, out));
            a[0] = out[0];
            a[1] = out[1];
        }
        return LR_OK;
    }
    // G groups per pass, the highest degrees first: G * batch <= max_batch, so no pool grows beyond what a call at max_batch needs
    const int G = std::min(degree - 1, std::max(1, pl->max_batch / batch));
    for (int top = degree; top > 1;) {
        const int g = std::min(G, top - 1), members = g * batch;
        LR_TRY(pl->bfvP.ensure(cQ, (size_t)2 * members * s));
        u64 *const p0 = pl->bfvP.d, *const p1 = pl->bfvP.d + (long long)members * s;        // back to back: the tail takes both at once
        const u64 *cx = ct[top]->d;
        long long cx_stride = ct[top]->stride();
        const lr_poly *keys[kBfvRelinFoldTerms];
        for (int i = 0; i < g; ++i) keys[i] = evks[top - i - 2];
        if (g > 1) {
            // the pass's input: ct[top], ct[top - 1], ... as one batch of g * batch members
            LR_TRY(pl->c2x.ensure(cQ, (size_t)members * s));
            MultiCopyLaunch M{};
            for (int i = 0; i < g; ++i) {
                M.src[i] = ct[top - i]->d; M.src_stride[i] = ct[top - i]->stride();
                M.dst[i] = pl->c2x.d + (long long)i * batch * s; M.dst_stride[i] = s;
            }
            M.count = g; M.batch = batch; M.n = n;
            LR_HIP(launch_multicopy(M, L1, cQ->stream));
            cx = pl->c2x.d;
            cx_stride = s;
        }
        LR_TRY(bfv_switch_keys_grouped(pl, batch, g, cx, cx_stride, keys, {{p0, p1}, {s, s}}));                            // :493, g degrees
        BfvRelinFoldLaunch F;
        for (int k = 0; k < 2; ++k) {
            F.base[k] = a[k].d; F.base_stride[k] = a[k].stride;
            F.out[k] = out[k].d; F.out_stride[k] = out[k].stride;
        }
        F.p[0] = p0; F.p[1] = p1; F.p_stride = s; F.group_stride = (long long)batch * s;
        F.terms = g;
        F.n = n;
        F.lp = cQ->d_lp;
        LR_HIP(launch_bfv_relin_fold(F, L1, batch, cQ->stream));                                                           // :494-495, g degrees
        a[0] = out[0];
        a[1] = out[1];
        top -= g;
    }
    return LR_OK;
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_bfv_relinearize_deg(lr_ckks_plan *pl, const lr_poly *const *ct, int degree, const lr_poly *const *evks, lr_poly *o0,
                                      lr_poly *o1) {
    return guarded([&]() -> int {
    if (!pl || !ct || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    if (degree < 1 || degree > 5) return fail(LR_ERR_ARG, "bfv relinearize: the degree must be 1 .. 5");
    for (int k = 0; k <= degree; ++k)
        if (!ct[k]) return fail(LR_ERR_ARG, "null argument");
    if (degree >= 2) {
        if (!evks) return fail(LR_ERR_ARG, "null argument");
        for (int k = 0; k + 2 <= degree; ++k)
            if (!evks[k]) return fail(LR_ERR_ARG, "null argument");
    }
    if (o0 == o1 || o0->d == o1->d) return fail(LR_ERR_ARG, "bfv relinearize: the two output polys must be distinct");
    for (int k = 2; k <= degree; ++k)
        if (ct[k] == o0 || ct[k] == o1 || ct[k]->d == o0->d || ct[k]->d == o1->d)
            return fail(LR_ERR_ARG, "bfv relinearize: an output must not be a component of degree 2 or more");
    if (o0 == ct[1] || o0->d == ct[1]->d || o1 == ct[0] || o1->d == ct[0]->d)
        return fail(LR_ERR_ARG, "bfv relinearize: an output must not be the other component's input");
    const int level = pl->cQ->h.L() - 1, batch = ct[0]->batch;
    if (batch > pl->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the plan's max_batch");
    for (int k = 0; k <= degree; ++k) LR_TRY(check_ct(pl, level, ct[k], batch));
    for (const lr_poly *p : {(const lr_poly *)o0, (const lr_poly *)o1}) LR_TRY(check_ct(pl, level, p, batch));
    const int alpha = pl->dec->alpha, beta = (level + 1 + alpha - 1) / alpha;
    for (int k = 0; k + 2 <= degree; ++k)
        if (evks[k]->N != pl->cQ->h.N || evks[k]->batch < 2 * beta || evks[k]->limbs < pl->cQ->h.L() + pl->cP->h.L())
            return fail(LR_ERR_SHAPE, "evaluation key: need batch >= 2*beta and |Q|+|P| limbs");
    return relin_core(pl, ct, degree, evks, o0, o1);
    });
}
