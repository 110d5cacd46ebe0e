// lr_abi_ckks_eval.cpp -- C ABI: the element side of ckks.Evaluator on an lr_ckks_plan (or, for the two streaming passes, on a context),
// over the key switch of lr_abi_ckks.cpp: lr_ckks_rotate, lr_ckks_mulrelin, lr_ckks_mul_norelin, lr_ckks_mul_plain, lr_ckks_rescale,
// lr_ckks_rotate_chain, lr_ckks_lincomb, lr_ckks_combine and lr_ckks_power_basis.  The scalar side of the last three -- levels, scales and
// per-limb words -- is lr_abi_ckks_scalar.cpp; the kernels of the last four are lr_ckks_eval.hip.
//   lr_ckks_lincomb        res = c0 + sum_k c_k ct_k for ciphertexts of degree 1, the leaf of the reference's polynomial evaluation
//                          (evaluatePolyFromPowerBasis, ckks/polynomial_evaluation.go:142-159): one streaming pass per sixteen terms
//   lr_ckks_combine        out = a (+|-) b for ciphertexts of any scale, level and degree, evaluator.Add / AddNoMod / Sub / SubNoMod through
//                          evaluateInPlace (ckks/evaluator.go:153-342), and the steps of the same shape between the products of polynomial
//                          and Chebyshev evaluation: one streaming pass
//   lr_ckks_rotate_chain   a chain of evaluator.permuteNTT steps (ckks/evaluator.go:1452-1471) as one call.  Over a state (a0, a1) on
//                          Q[0..level], NTT domain, step i with Galois element g_i and key K_i is
//     (e0, e1) = (PermuteNTT(a0, g_i), PermuteNTT(a1, g_i))     (p0, p1) = switchKeysInPlace(level, e1, K_i)     (r0, r1) = (CRed(e0 + p0), p1)
//     replace:     (a0, a1) <- (r0, r1)                               rotateColumnsPow2, :1414-1423
//     accumulate:  (a0, a1) <- (CRed(r0 + a0), CRed(r1 + a1))         RotateColumns(ct, ., tmp); Add(ct, tmp, ct): the slot-sum loop
//                          The fused route of an accumulating chain makes ONE pass in front of the key switch (launch_ckks_chain_step: the key
//                          switch's input and the first component's addend, the running sum already in it) and hands the running second
//                          component to the key switch's last pass as its other addend: no Add is left.  The composed route is
//                          ckks_rotate_step per step -- lr_ckks_rotate's body -- and two LR_ADD when accumulating; a replacing chain, which
//                          has no Add to lose, always takes it (chain_route).  Same bits on both for a state in [0, q).
//   lr_ckks_power_basis    the power basis of the reference's polynomial and Chebyshev evaluation, C[n] = C[ceil(n/2)] * C[n >> 1]
//                          (computePowerBasis, ckks/polynomial_evaluation.go:76-93) and C[n] = 2 C[a] C[b] - C[a - b] (computePowerBasisCheby,
//                          ckks/chebyshev_evaluation.go:60-101), as one call.  The merged route runs the products of one depth of the basis
//                          -- they share no data, one level and one key -- as ONE MulRelin over products * batch members read through a
//                          pointer table, the divisions on the staging pair it writes, and one tail pass (launch_ckks_basis_tail) that puts
//                          every C[n] where the caller wants it.  The composed route is lr_ckks_mulrelin, lr_ckks_rescale and
//                          lr_ckks_combine per product.  Same bits on both for inputs in [0, q).
#include "lr_host.hpp"

namespace lr_host {
namespace {

// a refusal under its entry point's name
struct Refuse {
    const char *who;
    int operator()(int code, const char *what) const { return fail(code, std::string(who) + what); }
};

// the words a poly spans, from its first to one past the last of its last member
struct PolySpan {
    const u64 *lo, *hi;
};
PolySpan poly_span(const lr_poly *p) { return {p->d, p->d + (long long)(p->batch - 1) * p->stride() + (long long)p->alloc_limbs * (long long)p->N}; }
bool overlap(const PolySpan &a, const PolySpan &b) { return a.lo < b.hi && b.lo < a.hi; }
// the words of two polys overlap
bool overlap(const lr_poly *a, const lr_poly *b) { return overlap(poly_span(a), poly_span(b)); }

// the very poly: the in-place case of the reference (the same component of the same ciphertext)
bool same_poly(const lr_poly *p, const lr_poly *o) { return p == o || (p->d == o->d && p->batch == o->batch && p->stride() == o->stride()); }

// THE strided operand fill of a TensorLaunch: the four polys of ct0 x ct1
void tensor_operands(TensorLaunch &T, const lr_poly *a0, const lr_poly *a1, const lr_poly *b0, const lr_poly *b1) {
    T.a0 = a0->d; T.a1 = a1->d; T.b0 = b0->d; T.b1 = b1->d;
    T.a0_stride = a0->stride(); T.a1_stride = a1->stride(); T.b0_stride = b0->stride(); T.b1_stride = b1->stride();
}

// the pools of a rotation at `level`: the permuted components and the key switch's accumulators, `batch` polys each
int ensure_rotate_pools(lr_ckks_plan *pl, int level, int batch) {
    const long long s = (long long)(level + 1) * (long long)pl->cQ->h.N;
    for (Pool *p : {&pl->c0, &pl->c2x, &pl->q1, &pl->q2}) LR_TRY(p->ensure(pl->cQ, (size_t)batch * s));
    return LR_OK;
}

// permuteNTT (ckks/evaluator.go:1448-1468) on components: lr_ckks_rotate, and each step of a composed chain.  The two trailing Context
// calls (:1466-1467) ride on the last ModDown pass.  The pools are ensure_rotate_pools'.
int ckks_rotate_step(lr_ckks_plan *pl, int level, int batch, const Comp (&in)[2], const Comp (&out)[2], u64 gen, const lr_poly *key) {
    lr_context *cQ = pl->cQ;
    const int L1 = level + 1;
    const long long s = (long long)L1 * (long long)cQ->h.N;
    const ComponentPair ins = component_pair(in[0].d, in[0].stride, in[1].d, in[1].stride, batch);
    if (batch == 1 && !pl->opt.no_pair && ins) {
        // one ciphertext: both components in one launch, the strides are the distances between them (see ks_ntt_tail)
        LR_TRY(run_permute_ntt(cQ, L1, 2, in[0].d, ins.stride, pl->c0.d, component_distance(pl->c0.d, pl->c2x.d), gen));    // :1458-1459
    } else {
        LR_TRY(run_permute_ntt(cQ, L1, batch, in[0].d, in[0].stride, pl->c0.d, s, gen));    // :1458
        LR_TRY(run_permute_ntt(cQ, L1, batch, in[1].d, in[1].stride, pl->c2x.d, s, gen));   // :1459
    }
    KeySwitchEpilogue fin{out[0].d, out[1].d, out[0].stride, pl->c0.d, nullptr, s};
    fin.out1_stride = out[1].stride;
    return switch_keys_core(pl, level, batch, pl->c2x.d, s, key, {{pl->q1.d, pl->q2.d}, {s, s}}, &fin);   // :1464-1467
}

// A fused or merged route is open at all: the plan and its context do not ask for the call-by-call shape (lr_options::no_epilogue), the key
// switch's last pass takes addends inside the forward transform (ntt_epilogue_ok), and the batch fits the grid of the routes' own passes
bool fused_routes_open(const lr_ckks_plan *pl, int batch) { return !plan_call_by_call(pl) && ntt_epilogue_ok(pl->cQ) && batch <= 32767; }

enum class ChainRoute { Fused, Composed };
// THE route decision of a CKKS chain.  An accumulating chain takes the fused step wherever the key switch's last pass
// takes addends inside the forward transform (ntt_epilogue_ok), unless the plan or its context asks for the call-by-call shape
// (lr_options::no_epilogue); a batch beyond the step pass's grid goes call by call as well.  A REPLACING chain is composed everywhere, as
// measured (one MI355X, DESIGN.md 6.2, the fused step against the RotateColumnsPow2 host loop in the same run, medians of 5): the pass in
// front of the key switch only stands for the two gathers that lr_ckks_rotate launches anyway, and no regime beat the host loop by more
// than the spread of the repeated medians -- PN15QP880 top level, one ciphertext 2272.9 us against 2276.8 (spread 18 and 33), 256
// ciphertexts 159.87 ms against 159.32 (0.68 and 0.79); PN16QP1761 top level, one ciphertext 7852.5 us against 7871.5 (32 and 34), 64
// ciphertexts 225.89 ms against 224.06 (1.10 and 1.72).  The slot sum is where the Add disappears: 2284.0 us against 2407.0 and 163.64 ms
// against 177.37 at PN15QP880, 7777.2 us against 8136.2 and 230.95 ms per 64 against 245.27 at PN16QP1761.
ChainRoute chain_route(const lr_ckks_plan *pl, int batch, bool accumulate) {
    if (!accumulate) return ChainRoute::Composed;
    if (!fused_routes_open(pl, batch)) return ChainRoute::Composed;
    return ChainRoute::Fused;
}

// the chain itself; every argument checked
int chain_core(lr_ckks_plan *pl, int level, const lr_poly *c0, const lr_poly *c1, int n_steps, const u64 *gens, const lr_poly *const *keys,
               bool accumulate, lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = pl->cQ;
    const int batch = c0->batch, L1 = level + 1, n = (int)cQ->h.N;
    const long long s = (long long)L1 * n;
    LR_TRY(begin_pipeline(pl));
    const bool fused = chain_route(pl, batch, accumulate) == ChainRoute::Fused;
    Comp a[2] = {c0, c1};
    const Comp out[2] = {o0, o1};
    // A replacing step's inputs are dead once they are permuted (both gathers come before the key switch writes anything): every step
    // writes the caller's outputs, in place from the second step on, whichever polys they are.  An accumulating step reads its state
    // again while it writes -- the fused route in the key switch's last pass, the composed one in its two Adds -- so there an output
    // over the OTHER component's input needs the state to start as a copy, and the fused route keeps the state off its destination.
    const bool crossed = out[0].d == a[1].d || out[1].d == a[0].d;
    const bool pools = accumulate || (crossed && n_steps == 0);
    if (pools)
        for (Pool *p : {&pl->bfvP, &pl->chainP}) LR_TRY(p->ensure(cQ, (size_t)2 * batch * s));
    LR_TRY(ensure_rotate_pools(pl, level, batch));
    u64 *const pair[2] = {pl->bfvP.d, pl->chainP.d};       // each [2][batch][level + 1][N]
    const KeySwitchAcc acc{{pl->q1.d, pl->q2.d}, {s, s}};
    auto copy = [&](const Comp &in, const Comp &dst) -> int {
        return in.d == dst.d ? (int)LR_OK : run_ewise(cQ, LR_COPY, L1, batch, in.d, in.stride, nullptr, 0, dst.d, dst.stride, nullptr);
    };
    int next = 0;      // the pool pair the next accumulating step writes; the state is never there
    if (pools && crossed) {
        for (int k = 0; k < 2; ++k) {
            const Comp dst(pair[1] + (long long)k * batch * s, s);
            LR_TRY(copy(a[k], dst));
            a[k] = dst;
        }
    }
    if (n_steps == 0) {
        for (int k = 0; k < 2; ++k) LR_TRY(copy(a[k], out[k]));
        return LR_OK;
    }
    for (int i = 0; i < n_steps; ++i) {
        const bool last = i == n_steps - 1;
        const Comp p[2] = {Comp(pair[next], s), Comp(pair[next] + (long long)batch * s, s)};
        if (fused) {
            // (accumulating: chain_route sends no replacing chain here)
            const Comp dst[2] = {last ? out[0] : p[0], last ? out[1] : p[1]};
            CkksChainStepLaunch S;
            S.a0 = a[0].d; S.a0_stride = a[0].stride; S.a1 = a[1].d; S.a1_stride = a[1].stride;
            S.plus0 = pl->c0.d; S.cx = pl->c2x.d; S.plus_stride = S.cx_stride = s;
            S.n = n; S.logn = (int)cQ->h.logN;
            S.gen = (u32)(gens[i] & ((cQ->h.N << 1) - 1));
            S.lp = cQ->d_lp;
            LR_HIP(launch_ckks_chain_step(S, L1, batch, cQ->stream));                                                 // :1458-1459 and Add, first component
            // The running second component is the last pass's other addend.  Where that pass would write the poly it adds -- a one-step
            // chain in place -- the result goes through the pool and is copied once: the transform epilogue and submul_kernel both load
            // the addend of an element before the same lane stores it, but nothing of the chain should hang on every variant of the
            // transform kernels keeping that order, for the sake of one copy in a chain of one step.
            const Comp w1 = dst[1].d == a[1].d ? p[1] : dst[1];
            KeySwitchEpilogue fin{dst[0].d, w1.d, dst[0].stride, pl->c0.d, a[1].d, s};
            fin.out1_stride = w1.stride;
            fin.plus1_stride = a[1].stride;
            LR_TRY(switch_keys_core(pl, level, batch, pl->c2x.d, s, keys[i], acc, &fin));                             // :1464-1467 and Add, second component
            LR_TRY(copy(w1, dst[1]));
            a[0] = dst[0];
            a[1] = dst[1];
            next ^= 1;
            continue;
        }
        // an accumulating step rotates into a pool pair and adds the state to it
        const Comp r[2] = {accumulate ? p[0] : out[0], accumulate ? p[1] : out[1]};
        LR_TRY(ckks_rotate_step(pl, level, batch, a, r, gens[i], keys[i]));                                           // :1458-1467
        if (accumulate)
            for (int k = 0; k < 2; ++k)
                LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, a[k].d, a[k].stride, r[k].d, r[k].stride, out[k].d, out[k].stride, nullptr));     // Add(ct, tmp, ct)
        a[0] = out[0];
        a[1] = out[1];
    }
    return LR_OK;
}

}  // namespace

// ckks/evaluator.go:1080-1104 after the argument checks: T holds the four operands (strided or through a pointer table)
int mulrelin_core(lr_ckks_plan *pl, int level, int batch, TensorLaunch T, const lr_poly *evk, u64 *o0, u64 *o1, long long o_stride) {
    lr_context *cQ = pl->cQ;
    LR_TRY(begin_pipeline(pl));
    const int n = (int)cQ->h.N, L1 = level + 1;
    const long long s = (long long)L1 * n;
    for (Pool *p : {&pl->c0, &pl->c1, &pl->c2x, &pl->q1, &pl->q2}) LR_TRY(p->ensure(cQ, (size_t)batch * s));
    // :1080-1095: MForm x2, MulCoeffsMontgomery x3, MulCoeffsMontgomeryAndAdd, one pass
    T.c0 = pl->c0.d; T.c1 = pl->c1.d; T.c2 = pl->c2x.d;
    T.c_stride = T.c1_stride = T.c2_stride = s;
    T.n = n;
    T.lp = cQ->d_lp;
    LR_HIP(launch_tensor(T, L1, batch, cQ->stream));
    // :1101 key switch of the degree-2 part, :1103-1104 the two additions fused into its last pass
    KeySwitchEpilogue fin{o0, o1, o_stride, pl->c0.d, pl->c1.d, s};
    return switch_keys_core(pl, level, batch, pl->c2x.d, s, evk, {{pl->q1.d, pl->q2.d}, {s, s}}, &fin);
}

namespace {

// one level of Rescale's loop on both components, each checked (check_rescale); the device is current
int ckks_rescale_core(lr_context *c, lr_poly *c0, lr_poly *c1) {
    // ckks/evaluator.go:958-960 divides the two components one after the other.  They are independent, and at a small batch every
    // launch of one component leaves most of the chip idle: where the two polys can be addressed as ONE batch -- base + p * stride
    // reaches both, i.e. always for one poly each (stride = the distance between them) and for batches laid out back to back --
    // every launch carries both (PN15QP880, one ciphertext: 121 -> 66 us).
    lr_poly *lo = c0->d <= c1->d ? c0 : c1, *hi = lo == c0 ? c1 : c0;
    const bool same_shape = c0->limbs == c1->limbs && c0->batch == c1->batch && c0->N == c1->N && c0->d != c1->d;
    const ComponentPair pair = component_pair(lo->d, lo->stride(), hi->d, hi->stride(), lo->batch);
    const bool one_each = pair.kind == ComponentPair::OneEach && pair.stride >= (long long)lo->limbs * (long long)lo->N;
    if (!c->opt.rescale_unpaired && same_shape && (one_each || pair.kind == ComponentPair::BackToBack) &&
        (long long)c0->batch * 2 * c0->limbs <= c->opt.pair_max_workgroups) {
        lr_poly both = *lo;
        both.owned = false;
        both.batch = 2 * lo->batch;
        both.stride_words = pair.stride;
        LR_TRY(rescale_ntt_domain(c, &both, true));
        c0->limbs = c1->limbs = both.limbs;
        return LR_OK;
    }
    LR_TRY(rescale_ntt_domain(c, c0, true));
    return rescale_ntt_domain(c, c1, true);
}

enum class BasisRoute { Merged, Composed };
// THE route decision of a power basis; `widest` = the products of the call's largest chunk.  The merged route needs the
// key switch's last pass inside the forward transform (ntt_epilogue_ok) and is not taken where the plan or its context asks for the
// call-by-call shape (lr_options::no_epilogue); a batch beyond the tail pass's grid goes product by product as well, and so does a call
// without a chunk of two products: there is nothing to merge.  Measured (one MI355X, DESIGN.md 6.2, the call against MulRelin, Rescale
// and CkksCombine per product in the same run, medians of 5; PN15QP880 and PN16QP1761 at their top levels, 1, 8 and 32 ciphertexts on a
// plan of max_batch 32): the merged route is ahead by more than the spread at every shape timed but ONE -- the Chebyshev list of degree
// 9, whose widest chunk is a pair, at 8 ciphertexts on PN15QP880: 2669.1 (2630.9 - 2803.3) us merged against 2680.7 (2676.5 - 2704.9),
// level inside the spread; product by product, as recorded in profiles/r13, 2609.4 (2586.8 - 2781.5) against 2641.8 (2617.9 - 2716.8),
// level as well.  The rule below gives that shape the composed route and EXTRAPOLATES from it: other batches of 8 or more and the
// degrees 2^12 .. 2^14 with a pair as the widest chunk were not timed.  The same list at N = 2^16 is ahead merged in the recorded run
// (10311.9 (10191.6 - 10476.1) against 10700.3 us) and stays merged, and so does every pair inside a call that also has a wider
// chunk: sending those pairs product by product was measured and cost the degree-33 and degree-129 lists 3 to 8 % at PN15QP880 and 8
// ciphertexts.
BasisRoute basis_route(const lr_ckks_plan *pl, int batch, int widest) {
    if (!fused_routes_open(pl, batch)) return BasisRoute::Composed;
    if (widest < 2) return BasisRoute::Composed;
    if (widest == 2 && batch >= 8 && pl->cQ->h.logN <= 15) return BasisRoute::Composed;
    return BasisRoute::Merged;
}

// the two polys of C[x]: C[1] or an earlier output
struct Operands {
    const lr_poly *c1[2];
    lr_poly *const *outs[2];
    const std::map<u32, int> *at;
    const lr_poly *of(u32 x, int u) const { return x == 1 ? c1[u] : outs[u][at->find(x)->second]; }
};

// the two halves of a staging pair as polys: [2][members][limbs][N], back to back (the paired form of lr_ckks_rescale)
void stage_views(lr_context *cQ, u64 *stage, int members, int limbs, lr_poly half[2]) {
    const long long s = (long long)limbs * (long long)cQ->h.N;
    for (int u = 0; u < 2; ++u) {
        half[u] = lr_poly();
        half[u].ctx = cQ;
        half[u].device = cQ->device;
        half[u].N = cQ->h.N;
        half[u].d = stage + (long long)u * members * s;
        half[u].limbs = half[u].alloc_limbs = limbs;
        half[u].batch = members;
        half[u].stride_words = s;
    }
}

// one product from the existing calls: lr_ckks_mulrelin, lr_ckks_rescale, lr_ckks_combine.  An output holds level_after + 1 limbs, a
// product that is divided has more before its divisions: it goes through the plan's staging pair and the tail writes the output.
int composed_product(lr_ckks_plan *pl, const lr_ckks_basis_product &P, const u64 *mult, const u64 *add, const Operands &ops, const lr_poly *evk,
                     lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = pl->cQ;
    const int batch = o0->batch, n = (int)cQ->h.N;
    const long long s = (long long)(P.mul_level + 1) * n;
    const bool staged = P.n_rescales > 0;
    lr_poly v[2] = {*o0, *o1};      // views: the caller's logical limb counts are left alone
    v[0].owned = v[1].owned = false;
    v[0].limbs = v[1].limbs = P.mul_level + 1;
    if (staged) {
        LR_TRY(pl->basisS.ensure(cQ, (size_t)2 * batch * s));
        stage_views(cQ, pl->basisS.d, batch, P.mul_level + 1, v);
    }
    TensorLaunch T;
    tensor_operands(T, ops.of(P.a, 0), ops.of(P.a, 1), ops.of(P.b, 0), ops.of(P.b, 1));
    LR_TRY(mulrelin_core(pl, P.mul_level, batch, T, evk, v[0].d, v[1].d, v[0].stride()));                        // MulRelinNew :87
    for (int r = 0; r < P.n_rescales; ++r) LR_TRY(ckks_rescale_core(cQ, &v[0], &v[1]));                           // Rescale :89
    const lr_poly *const a[2] = {staged ? &v[0] : o0, staged ? &v[1] : o1}, *const b[2] = {ops.c1[0], ops.c1[1]};
    lr_poly *const out[2] = {o0, o1};
    if (P.tail == 0) {
        if (!staged) return LR_OK;
        for (int u = 0; u < 2; ++u)
            LR_TRY(run_ewise(cQ, LR_COPY, P.level_after + 1, batch, v[u].d, v[u].stride(), nullptr, 0, out[u]->d, out[u]->stride(), nullptr));
        return LR_OK;
    }
    if (P.tail == 1) {                                                                                             // Add :92, Sub :98
        const u64 *ma = P.mult_side == 1 ? mult : nullptr, *mb = P.mult_side == 2 ? mult : nullptr;
        return lr_ckks_combine(cQ, LR_SUB, P.level_after, 1, a, 1, b, 1, ma, ma, mb, mb, nullptr, nullptr, out);
    }
    return lr_ckks_combine(cQ, LR_SUB, P.level_after, 1, a, 0, nullptr, 1, nullptr, nullptr, nullptr, nullptr, add, add, out);      // Add :92, AddConst :96
}

// `count` products of one group -- one layer, one mul_level, one n_rescales -- as one MulRelin, its divisions and one tail pass
int merged_chunk(lr_ckks_plan *pl, const lr_ckks_basis_product *products, const int *which, int count, const u64 *mult, const u64 *add,
                 int row_words, const Operands &ops, const lr_poly *evk) {
    lr_context *cQ = pl->cQ;
    const lr_ckks_basis_product &G = products[which[0]];
    const int batch = ops.c1[0]->batch, members = count * batch, n = (int)cQ->h.N, row = G.level_after + 1;
    const long long s = (long long)(G.mul_level + 1) * n;
    // the chunk's tables: [4 * members] operand pointers, [count] entries, [count][row] multiplier words, [count][row] addend words
    const size_t off_entries = (size_t)4 * members * sizeof(u64 *), off_mult = off_entries + (size_t)count * sizeof(BasisTailProduct),
                 off_add = off_mult + (size_t)count * row * sizeof(u64), bytes = off_add + (size_t)count * row * sizeof(u64);
    TableSlots::Slot *slot = nullptr;
    LR_TRY(pl->basisT.take(cQ->stream, bytes, &slot));
    const u64 **tab = reinterpret_cast<const u64 **>(slot->h);
    BasisTailProduct *entries = reinterpret_cast<BasisTailProduct *>(slot->h + off_entries);
    u64 *h_mult = reinterpret_cast<u64 *>(slot->h + off_mult), *h_add = reinterpret_cast<u64 *>(slot->h + off_add);
    for (int k = 0; k < count; ++k) {
        const int p = which[k];
        const lr_ckks_basis_product &P = products[p];
        const lr_poly *opnd[4] = {ops.of(P.a, 0), ops.of(P.a, 1), ops.of(P.b, 0), ops.of(P.b, 1)};
        for (int b = 0; b < batch; ++b)
            for (int j = 0; j < 4; ++j) tab[4 * ((size_t)k * batch + b) + j] = opnd[j]->d + (long long)b * opnd[j]->stride();
        entries[k] = BasisTailProduct{{ops.outs[0][p]->d, ops.outs[1][p]->d}, ops.outs[0][p]->stride(), P.tail, P.mult_side};
        std::copy(mult + (size_t)p * row_words, mult + (size_t)p * row_words + row, h_mult + (size_t)k * row);
        std::copy(add + (size_t)p * row_words, add + (size_t)p * row_words + row, h_add + (size_t)k * row);
    }
    LR_TRY(pl->basisS.ensure(cQ, (size_t)2 * members * s));
    LR_TRY(pl->basisT.send(cQ->stream, slot, bytes));
    u64 *const stage = pl->basisS.d;
    TensorLaunch T{};
    T.table = reinterpret_cast<const u64 *const *>(slot->d);
    LR_TRY(mulrelin_core(pl, G.mul_level, members, T, evk, stage, stage + (long long)members * s, s));            // MulRelinNew :87 of every product
    // Rescale's loop :945-961 on the staging pair: its halves lie back to back, the paired form of lr_ckks_rescale
    lr_poly half[2];
    stage_views(cQ, stage, members, G.mul_level + 1, half);
    for (int r = 0; r < G.n_rescales; ++r) LR_TRY(ckks_rescale_core(cQ, &half[0], &half[1]));
    BasisTailLaunch L;
    L.stage = stage;
    L.stage_stride = s;
    for (int u = 0; u < 2; ++u) {
        L.c1[u] = ops.c1[u]->d;
        L.c1_stride[u] = ops.c1[u]->stride();
    }
    L.products = reinterpret_cast<const BasisTailProduct *>(slot->d + off_entries);
    L.mult = reinterpret_cast<const u64 *>(slot->d + off_mult);
    L.add = reinterpret_cast<const u64 *>(slot->d + off_add);
    L.row = row;
    L.batch = batch;
    L.n = n;
    L.lp = cQ->d_lp;
    LR_HIP(launch_ckks_basis_tail(L, row, count, cQ->stream));                                                     // :92-99, and C[n] to its polys
    return LR_OK;
}

}  // namespace
}  // namespace lr_host

// permuteNTT (ckks/evaluator.go:1448-1468): RotateColumns with a specific rotation key / Conjugate.
// gen = the Galois element (ring.PermuteNTTIndex's `gen^power`): one ckks_rotate_step into the caller's outputs.
extern "C" int lr_ckks_rotate(lr_ckks_plan *pl, int level, const lr_poly *c0, const lr_poly *c1, uint64_t gen, const lr_poly *rotkey,
                              lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int {
    if (!pl || !c0 || !c1 || !rotkey || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    const int batch = c0->batch;
    LR_TRY(check_call(pl, level, batch, {c0, c1, o0, o1}));
    if (o0->stride() != o1->stride()) return fail(LR_ERR_SHAPE, "output polys must share their stride");
    LR_TRY(begin_pipeline(pl));
    LR_TRY(ensure_rotate_pools(pl, level, batch));
    return ckks_rotate_step(pl, level, batch, {c0, c1}, {o0, o1}, gen, rotkey);
    });
}

extern "C" int lr_ckks_mulrelin(lr_ckks_plan *pl, int level, const lr_poly *a0, const lr_poly *a1, const lr_poly *b0,
                                const lr_poly *b1, const lr_poly *evk, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int {
    if (!pl || !a0 || !a1 || !b0 || !b1 || !evk || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    const int batch = a0->batch;
    LR_TRY(check_call(pl, level, batch, {a0, a1, b0, b1, o0, o1}));
    if (o0->stride() != o1->stride()) return fail(LR_ERR_SHAPE, "output polys must share their stride");
    TensorLaunch T;
    tensor_operands(T, a0, a1, b0, b1);
    return mulrelin_core(pl, level, batch, T, evk, o0->d, o1->d, o0->stride());
    });
}

// MulRelin with evakey == nil (ckks/evaluator.go:1038-1111): the degree-2 tensor, no key switch.  The squaring branch
// (:1083-1088, c1 = 2 c0 c1 by AddLvl) and the regular one (:1090-1096, MulCoeffsMontgomeryAndAddLvl) produce the same canonical
// residues when ct0 == ct1, so one kernel serves both.  Outputs may alias the inputs (the reference goes through its pools then).
extern "C" int lr_ckks_mul_norelin(lr_ckks_plan *pl, int level, const lr_poly *a0, const lr_poly *a1, const lr_poly *b0,
                                   const lr_poly *b1, lr_poly *o0, lr_poly *o1, lr_poly *o2) {
    return guarded([&]() -> int {
    if (!pl || !a0 || !a1 || !b0 || !b1 || !o0 || !o1 || !o2) return fail(LR_ERR_ARG, "null argument");
    const int batch = a0->batch;
    LR_TRY(check_call(pl, level, batch, {a0, a1, b0, b1, o0, o1, o2}));
    lr_context *cQ = pl->cQ;
    LR_HIP(hipSetDevice(cQ->device));
    TensorLaunch T;
    tensor_operands(T, a0, a1, b0, b1);
    T.c0 = o0->d; T.c1 = o1->d; T.c2 = o2->d;
    T.c_stride = o0->stride(); T.c1_stride = o1->stride(); T.c2_stride = o2->stride();
    T.n = (int)cQ->h.N;
    T.lp = cQ->d_lp;
    LR_HIP(launch_tensor(T, level + 1, batch, cQ->stream));
    return LR_OK;
    });
}

// MulRelin, plaintext x ciphertext (ckks/evaluator.go:1113-1131): out_k = MRed(MForm(pt), ct_k), k = 0, 1
extern "C" int lr_ckks_mul_plain(lr_ckks_plan *pl, int level, const lr_poly *pt, const lr_poly *c0, const lr_poly *c1,
                                 lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int {
    if (!pl || !pt || !c0 || !c1 || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    const int batch = c0->batch;
    LR_TRY(check_call(pl, level, batch, {c0, c1, o0, o1}));
    if (pt->N != pl->cQ->h.N || pt->limbs < level + 1 || (pt->batch != batch && pt->batch != 1)) return fail(LR_ERR_SHAPE, "plaintext: limbs or batch");
    lr_context *cQ = pl->cQ;
    LR_HIP(hipSetDevice(cQ->device));
    const int n = (int)cQ->h.N, L1 = level + 1;
    const long long s = (long long)L1 * n;
    LR_TRY(pl->c0.ensure(cQ, (size_t)pt->batch * s));
    LR_TRY(run_ewise(cQ, LR_MFORM, L1, pt->batch, pt->d, pt->stride(), nullptr, 0, pl->c0.d, s, nullptr));            // :1129
    const long long ms = pt->batch == 1 && batch > 1 ? 0 : s;
    LR_TRY(run_ewise(cQ, LR_MUL_MONT, L1, batch, pl->c0.d, ms, c0->d, c0->stride(), o0->d, o0->stride(), nullptr));   // :1130
    return run_ewise(cQ, LR_MUL_MONT, L1, batch, pl->c0.d, ms, c1->d, c1->stride(), o1->d, o1->stride(), nullptr);    // :1131
    });
}

extern "C" int lr_ckks_rescale(lr_ckks_plan *pl, lr_poly *c0, lr_poly *c1) {
    return guarded([&]() -> int {
    if (!pl || !c0 || !c1) return fail(LR_ERR_ARG, "null argument");
    lr_context *c = pl->cQ;
    LR_TRY(check_rescale(c, c0));
    LR_TRY(check_rescale(c, c1));
    LR_HIP(hipSetDevice(c->device));
    return ckks_rescale_core(c, c0, c1);
    });
}

extern "C" int lr_ckks_rotate_chain(lr_ckks_plan *pl, int level, const lr_poly *c0, const lr_poly *c1, int n_steps, const uint64_t *gens,
                                    const lr_poly *const *keys, int accumulate, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int {
    const Refuse refuse{"ckks rotate chain: "};
    // LR_ERR_ARG
    if (!pl || !c0 || !c1 || !o0 || !o1) return refuse(LR_ERR_ARG, "null argument");
    if (n_steps < 0) return refuse(LR_ERR_ARG, "negative step count");
    if (n_steps > 0 && (!gens || !keys)) return refuse(LR_ERR_ARG, "null argument");
    for (int i = 0; i < n_steps; ++i) {
        if (!keys[i]) return refuse(LR_ERR_ARG, "null argument");
        if (!(gens[i] & 1)) return refuse(LR_ERR_ARG, "a Galois element must be odd");
    }
    if (o0 == o1 || o0->d == o1->d) return refuse(LR_ERR_ARG, "the two output polys must be distinct");
    // LR_ERR_SHAPE
    LR_TRY(check_call(pl, level, c0->batch, {c0, c1, o0, o1}));
    for (int i = 0; i < n_steps; ++i)
        if (!switching_key_ok(pl, level, keys[i])) return refuse(LR_ERR_SHAPE, "rotation key: need batch >= 2*beta and |Q|+|P| limbs");
    if (pl->cQ->h.N < 2 || pl->cQ->h.logN > 30) return refuse(LR_ERR_UNSUPPORTED, "ring degree");
    return chain_core(pl, level, c0, c1, n_steps, gens, keys, accumulate != 0, o0, o1);
    });
}

extern "C" int lr_ckks_lincomb(lr_context *c, int level, int n_terms, const lr_poly *const *terms_c0, const lr_poly *const *terms_c1,
                               const uint8_t *has_pre, const uint64_t *pre, const uint64_t *lo, const uint64_t *hi, const uint64_t *add_lo,
                               const uint64_t *add_hi, int accumulate, lr_poly *out_c0, lr_poly *out_c1) {
    return guarded([&]() -> int {
    const Refuse refuse{"CKKS linear combination: "};
    // LR_ERR_ARG
    if (!c || !out_c0 || !out_c1) return refuse(LR_ERR_ARG, "null argument");
    if (n_terms < 0) return refuse(LR_ERR_ARG, "n_terms is negative");
    if (n_terms > 0 && (!terms_c0 || !terms_c1 || !has_pre || !pre || !lo || !hi)) return refuse(LR_ERR_ARG, "null argument");
    for (int k = 0; k < n_terms; ++k)
        if (!terms_c0[k] || !terms_c1[k]) return refuse(LR_ERR_ARG, "a term is null");
    if ((add_lo == nullptr) != (add_hi == nullptr)) return refuse(LR_ERR_ARG, "add_lo and add_hi come together or not at all");
    if (out_c0 == out_c1 || overlap(out_c0, out_c1)) return refuse(LR_ERR_ARG, "the two components of the receiver share memory");
    for (int k = 0; k < n_terms; ++k)
        for (const lr_poly *t : {terms_c0[k], terms_c1[k]})
            if (overlap(t, out_c0) || overlap(t, out_c1)) return refuse(LR_ERR_ARG, "a term shares memory with the receiver");
    // LR_ERR_SHAPE
    const int batch = out_c0->batch;
    const auto shape = [&](const lr_poly *p) -> int {
        if (p->N != c->h.N) return refuse(LR_ERR_SHAPE, "ring degree mismatch");
        if (level + 1 > p->limbs) return refuse(LR_ERR_SHAPE, "a poly has fewer limbs than level + 1");
        if (p->batch != batch) return refuse(LR_ERR_SHAPE, "every term and the receiver carry the same batch");
        return LR_OK;
    };
    if (level < 0 || level + 1 > c->h.L()) return refuse(LR_ERR_SHAPE, "level out of range");
    LR_TRY(shape(out_c0));
    LR_TRY(shape(out_c1));
    for (int k = 0; k < n_terms; ++k) {
        LR_TRY(shape(terms_c0[k]));
        LR_TRY(shape(terms_c1[k]));
    }
    if (batch > 32767) return refuse(LR_ERR_SHAPE, "batch above 32767");
    // LR_ERR_UNSUPPORTED
    if (c->h.N < 4) return refuse(LR_ERR_UNSUPPORTED, "ring degree below 4");

    if (n_terms == 0 && !add_lo && accumulate) return LR_OK;      // the receiver as it is
    LR_HIP(hipSetDevice(c->device));
    const int L1 = level + 1;
    // kLinCombTerms terms per pass, the constant on the first, every further pass on top of the receiver; within a pass as many limbs per
    // launch as its constants leave room for in the kernel arguments
    int first = 0;
    do {
        const int count = std::min(n_terms - first, kLinCombTerms);
        LinCombLaunch L;
        std::memset(&L, 0, sizeof L);
        for (int k = 0; k < count; ++k) {
            const lr_poly *t0 = terms_c0[first + k], *t1 = terms_c1[first + k];
            L.term[k] = LinCombTermRef{{t0->d, t1->d}, {t0->stride(), t1->stride()}};
            if (has_pre[first + k]) L.pre_mask |= 1u << k;
        }
        L.out[0] = out_c0->d;
        L.out[1] = out_c1->d;
        L.out_stride[0] = out_c0->stride();
        L.out_stride[1] = out_c1->stride();
        L.n = (int)c->h.N;
        L.count = count;
        L.accumulate = first > 0 || accumulate ? 1 : 0;
        L.has_add = first == 0 && add_lo ? 1 : 0;
        L.lp = c->d_lp;
        const int words = lincomb_limb_words(count, L.has_add), step = lincomb_limbs_per_launch(count, L.has_add);
        for (int limb0 = 0; limb0 < L1; limb0 += step) {
            const int limbs = std::min(step, L1 - limb0);
            L.limb0 = limb0;
            for (int y = 0; y < limbs; ++y) {
                u64 *w = L.k + (size_t)y * words;
                const int i = limb0 + y;
                if (L.has_add) {
                    *w++ = add_lo[i];
                    *w++ = add_hi[i];
                }
                for (int k = 0; k < count; ++k) {
                    const size_t at = (size_t)(first + k) * L1 + i;
                    *w++ = L.pre_mask >> k & 1u ? pre[at] : 0;
                    *w++ = lo[at];
                    *w++ = hi[at];
                }
            }
            LR_HIP(launch_ckks_lincomb(L, limbs, batch, c->stream));
        }
        first += count;
    } while (first < n_terms);
    return LR_OK;
    });
}

extern "C" int lr_ckks_combine(lr_context *c, int op, int level, int a_degree, const lr_poly *const *a, int b_degree, const lr_poly *const *b,
                               int double_a, const uint64_t *ma_lo, const uint64_t *ma_hi, const uint64_t *mb_lo, const uint64_t *mb_hi,
                               const uint64_t *add_lo, const uint64_t *add_hi, lr_poly *const *out) {
    return guarded([&]() -> int {
    const Refuse refuse{"CKKS combine: "};
    // LR_ERR_ARG
    if (!c || !out) return refuse(LR_ERR_ARG, "null argument");
    if (!a) return refuse(LR_ERR_ARG, "no operand given");
    if (op < LR_ADD || op > LR_SUB_NOMOD) return refuse(LR_ERR_ARG, "the operation is not LR_ADD, LR_ADD_NOMOD, LR_SUB or LR_SUB_NOMOD");
    if (a_degree < 0 || a_degree > 2 || (b && (b_degree < 0 || b_degree > 2))) return refuse(LR_ERR_ARG, "a degree is outside 0..2");
    const int deg_b = b ? b_degree : -1, comps = combine_comps(a_degree, deg_b);
    for (int u = 0; u <= a_degree; ++u)
        if (!a[u]) return refuse(LR_ERR_ARG, "a component is null");
    for (int u = 0; u <= deg_b; ++u)
        if (!b[u]) return refuse(LR_ERR_ARG, "a component is null");
    for (int u = 0; u < comps; ++u)
        if (!out[u]) return refuse(LR_ERR_ARG, "a component is null");
    if ((ma_lo == nullptr) != (ma_hi == nullptr) || (mb_lo == nullptr) != (mb_hi == nullptr) || (add_lo == nullptr) != (add_hi == nullptr))
        return refuse(LR_ERR_ARG, "the two words of a multiplier or of the constant come together or not at all");
    if (!b && mb_lo) return refuse(LR_ERR_ARG, "a multiplier of b without b");
    // out_u may be the very poly a_u or b_u; nothing else of the receiver may share memory with anything
    for (int u = 0; u < comps; ++u)
        for (int v = u + 1; v < comps; ++v)
            if (out[u] == out[v] || overlap(out[u], out[v])) return refuse(LR_ERR_ARG, "the components of the receiver share memory");
    for (int u = 0; u < comps; ++u) {
        for (int v = 0; v <= a_degree; ++v)
            if (overlap(a[v], out[u]) && !(u == v && same_poly(a[v], out[u])))
                return refuse(LR_ERR_ARG, "an operand shares memory with the receiver other than component by component in place");
        for (int v = 0; v <= deg_b; ++v)
            if (overlap(b[v], out[u]) && !(u == v && same_poly(b[v], out[u])))
                return refuse(LR_ERR_ARG, "an operand shares memory with the receiver other than component by component in place");
    }
    // LR_ERR_SHAPE
    if (level < 0 || level + 1 > c->h.L()) return refuse(LR_ERR_SHAPE, "level out of range");
    const int batch = out[0]->batch;
    const auto shape = [&](const lr_poly *p, bool operand) -> int {
        if (p->N != c->h.N) return refuse(LR_ERR_SHAPE, "ring degree mismatch");
        if (level + 1 > p->limbs) return refuse(LR_ERR_SHAPE, "a poly has fewer limbs than level + 1");
        if (p->batch != batch && !(operand && p->batch == 1))
            return refuse(LR_ERR_SHAPE, "the receiver's components carry one batch, an operand that batch or 1");
        return LR_OK;
    };
    for (int u = 0; u < comps; ++u) LR_TRY(shape(out[u], false));
    for (int u = 0; u <= a_degree; ++u) LR_TRY(shape(a[u], true));
    for (int u = 0; u <= deg_b; ++u) LR_TRY(shape(b[u], true));
    if (batch > 32767) return refuse(LR_ERR_SHAPE, "batch above 32767");
    if ((long long)comps * batch > 65535) return refuse(LR_ERR_SHAPE, "batch above 21845 at degree 2");
    // LR_ERR_UNSUPPORTED
    if (c->h.N < 4) return refuse(LR_ERR_UNSUPPORTED, "ring degree below 4");

    LR_HIP(hipSetDevice(c->device));
    CombineLaunch L;
    std::memset(&L, 0, sizeof L);
    const auto stride = [&](const lr_poly *p) { return p->batch == 1 && batch > 1 ? 0ll : p->stride(); };       // one poly read by every member
    for (int u = 0; u <= a_degree; ++u) {
        L.a[u] = a[u]->d;
        L.a_stride[u] = stride(a[u]);
    }
    for (int u = 0; u <= deg_b; ++u) {
        L.b[u] = b[u]->d;
        L.b_stride[u] = stride(b[u]);
    }
    for (int u = 0; u < comps; ++u) {
        L.out[u] = out[u]->d;
        L.out_stride[u] = out[u]->stride();
    }
    L.n = (int)c->h.N;
    L.op = op;
    L.deg_a = a_degree;
    L.deg_b = deg_b;
    L.double_a = double_a ? 1 : 0;
    L.mult_a = ma_lo ? 1 : 0;
    L.mult_b = mb_lo ? 1 : 0;
    L.has_add = add_lo ? 1 : 0;
    L.lp = c->d_lp;
    for (int i = 0; i <= level; ++i) {
        u64 *w = L.k + (size_t)i * kCombineLimbWords;
        if (ma_lo) w[0] = ma_lo[i], w[1] = ma_hi[i];
        if (mb_lo) w[2] = mb_lo[i], w[3] = mb_hi[i];
        if (add_lo) w[4] = add_lo[i], w[5] = add_hi[i];
    }
    LR_HIP(launch_ckks_combine(L, level + 1, batch, c->stream));
    return LR_OK;
    });
}

extern "C" int lr_ckks_power_basis(lr_ckks_plan *pl, int n_products, const lr_ckks_basis_product *products, const uint64_t *mult,
                                   const uint64_t *add, int row_words, int c1_level, const lr_poly *c1_c0, const lr_poly *c1_c1,
                                   const lr_poly *evk, lr_poly *const *outs_c0, lr_poly *const *outs_c1) {
    return guarded([&]() -> int {
    const Refuse refuse{"CKKS power basis: "};
    // LR_ERR_ARG
    if (!pl || !c1_c0 || !c1_c1 || !evk) return refuse(LR_ERR_ARG, "null argument");
    if (n_products < 0) return refuse(LR_ERR_ARG, "negative product count");
    if (n_products > 0 && (!products || !mult || !add || !outs_c0 || !outs_c1)) return refuse(LR_ERR_ARG, "null argument");
    for (int k = 0; k < n_products; ++k)
        if (!outs_c0[k] || !outs_c1[k]) return refuse(LR_ERR_ARG, "an output is null");
    if (row_words < c1_level + 1) return refuse(LR_ERR_ARG, "row_words is below c1_level + 1");
    std::map<u32, int> at;
    for (int k = 0; k < n_products; ++k) {
        const lr_ckks_basis_product &P = products[k];
        const char *const kBad = "the schedule is not self-consistent";
        struct State { int level, layer; };
        State st[2];
        const u32 opnd[2] = {P.a, P.b};
        for (int j = 0; j < 2; ++j) {
            if (opnd[j] == 1) {
                st[j] = State{c1_level, 0};
                continue;
            }
            const auto it = at.find(opnd[j]);
            if (it == at.end()) return refuse(LR_ERR_ARG, kBad);            // neither C[1] nor an earlier product
            st[j] = State{products[it->second].level_after, products[it->second].layer};
        }
        if (P.n < 2 || at.count(P.n) || st[0].layer >= P.layer || st[1].layer >= P.layer || P.mul_level != std::min(st[0].level, st[1].level) ||
            P.tail < 0 || P.tail > 2 || P.mult_side < 0 || P.mult_side > 2 || P.n_rescales < 0 || P.n_rescales > P.mul_level ||
            P.level_after != P.mul_level - P.n_rescales || (P.tail == 1 && P.c != 1))
            return refuse(LR_ERR_ARG, kBad);
        at[P.n] = k;
    }
    {
        // no two outputs share memory, none shares memory with C[1]: by address, neighbours in the sorted order
        std::vector<PolySpan> spans;
        spans.reserve((size_t)2 * n_products);
        for (int k = 0; k < n_products; ++k) {
            spans.push_back(poly_span(outs_c0[k]));
            spans.push_back(poly_span(outs_c1[k]));
        }
        std::sort(spans.begin(), spans.end(), [](const PolySpan &x, const PolySpan &y) { return x.lo < y.lo; });
        for (size_t i = 1; i < spans.size(); ++i)
            if (spans[i].lo < spans[i - 1].hi) return refuse(LR_ERR_ARG, "two outputs share memory");
        for (const lr_poly *c : {c1_c0, c1_c1})
            for (const PolySpan &o : spans)
                if (overlap(poly_span(c), o)) return refuse(LR_ERR_ARG, "an output shares memory with C[1]");
    }
    // LR_ERR_SHAPE
    const int batch = c1_c0->batch;
    LR_TRY(check_batch(pl, batch));
    if (c1_level < 0 || c1_level + 1 > pl->cQ->h.L()) return refuse(LR_ERR_SHAPE, "level out of range");
    LR_TRY(check_cts(pl, c1_level, batch, {c1_c0, c1_c1}));
    for (int k = 0; k < n_products; ++k) {
        LR_TRY(check_cts(pl, products[k].level_after, batch, {outs_c0[k], outs_c1[k]}));
        if (outs_c0[k]->stride() != outs_c1[k]->stride()) return refuse(LR_ERR_SHAPE, "the two polys of an output must share their stride");
    }
    if (!switching_key_ok(pl, c1_level, evk)) return refuse(LR_ERR_SHAPE, "evaluation key: need batch >= 2*beta and |Q|+|P| limbs");
    if (n_products == 0) return LR_OK;
    if (pl->cQ->h.N < 4) return refuse(LR_ERR_UNSUPPORTED, "ring degree below 4");
    LR_TRY(begin_pipeline(pl));

    const Operands ops{{c1_c0, c1_c1}, {outs_c0, outs_c1}, &at};
    // the products of one layer that share mul_level and n_rescales form a group; layers in rising order, so every operand is ready
    std::vector<int> order((size_t)n_products);
    for (int k = 0; k < n_products; ++k) order[k] = k;
    const auto key_less = [&](int x, int y) {
        const lr_ckks_basis_product &X = products[x], &Y = products[y];
        if (X.layer != Y.layer) return X.layer < Y.layer;
        if (X.mul_level != Y.mul_level) return X.mul_level > Y.mul_level;
        return X.n_rescales < Y.n_rescales;
    };
    std::stable_sort(order.begin(), order.end(), key_less);
    const int per_chunk = std::max(1, std::min(pl->max_batch, 32767) / std::max(1, batch));
    std::vector<int> group_end;      // one past each group in `order`
    int widest = 1;
    for (int g0 = 0, g1; g0 < n_products; g0 = g1) {
        g1 = g0 + 1;
        while (g1 < n_products && !key_less(order[g0], order[g1])) ++g1;
        group_end.push_back(g1);
        widest = std::max(widest, std::min(per_chunk, g1 - g0));
    }
    if (basis_route(pl, batch, widest) == BasisRoute::Composed) {
        for (int k = 0; k < n_products; ++k)
            LR_TRY(composed_product(pl, products[k], mult + (size_t)k * row_words, add + (size_t)k * row_words, ops, evk, outs_c0[k], outs_c1[k]));
        return LR_OK;
    }
    int g0 = 0;
    for (int g1 : group_end) {
        for (int k0 = g0; k0 < g1; k0 += per_chunk) {
            const int count = std::min(per_chunk, g1 - k0), k = order[k0];
            // a chunk of one product has nothing to merge: the product as it stands, without the table and the staging pass
            if (count == 1) LR_TRY(composed_product(pl, products[k], mult + (size_t)k * row_words, add + (size_t)k * row_words, ops, evk, outs_c0[k], outs_c1[k]));
            else LR_TRY(merged_chunk(pl, products, &order[k0], count, mult, add, row_words, ops, evk));
        }
        g0 = g1;
    }
    return LR_OK;
    });
}
