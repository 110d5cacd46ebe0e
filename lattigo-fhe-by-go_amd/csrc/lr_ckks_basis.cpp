// lr_ckks_basis.cpp -- C ABI: the power basis of the reference's polynomial and Chebyshev evaluation, C[n] = C[ceil(n/2)] * C[n >> 1]
// (computePowerBasis, ckks/polynomial_evaluation.go:76-93) and C[n] = 2 C[a] C[b] - C[a - b] (computePowerBasisCheby,
// ckks/chebyshev_evaluation.go:60-101), and with them PowerOf2 (ckks/algorithms.go:9-31), which is computePowerBasis(2^k).
//   lr_ckks_power_basis_schedule   the scalar side, host only (no context, no device): which products, in the reference's order, and per
//                                  product the level, the Rescale loop's trip count, the scale and the words of the Chebyshev tail
//   lr_ckks_power_basis            the element side as one call.  The merged route runs the products of one depth of the basis -- they
//                                  share no data, one level and one key -- as ONE MulRelin over products * batch members read through a
//                                  pointer table, the divisions on the staging pair it writes, and one tail pass (lr_ckks_basis.hip) that
//                                  puts every C[n] where the caller wants it.  The composed route is lr_ckks_mulrelin, lr_ckks_rescale
//                                  and lr_ckks_combine per product.  Same bits on both for inputs in [0, q).
// The scalar words come from the restatements that exist: lr_ckks_combine_constants for Sub, lr_ckks_scalar.hpp for AddConst.
// The unit's name keeps it out of the lr_abi_*.cpp set that the shared sanitizer build links against its fixed launch stubs: the launcher
// it calls has a stand-in of its own (tests/cpp/ckks_basis_stub.cpp).
#include "lr_ckks_scalar.hpp"

namespace lr_host {
namespace {
using namespace ckks_scalar;

const char *const kWho = "CKKS power basis: ";
const char *const kWhoSched = "CKKS power basis schedule: ";

int refuse_sched(const char *what) { return fail(LR_ERR_ARG, std::string(kWhoSched) + what); }
int refuse(int code, const char *what) { return fail(code, std::string(kWho) + what); }

// the recursion of :78-92 / :70-99: a, then b, each only when not yet present (c is 0 or 1 and C[1] is always present)
struct Recursion {
    std::map<u32, int> at;               // n -> its product
    std::vector<u32> order;
    void want(u32 n) {
        if (n == 1 || at.count(n)) return;
        want((n + 1) >> 1);
        want(n >> 1);
        at[n] = (int)order.size();
        order.push_back(n);
    }
};

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
    if (pl->opt.no_epilogue || pl->cQ->opt.no_epilogue) return BasisRoute::Composed;
    if (!ntt_epilogue_ok(pl->cQ)) return BasisRoute::Composed;
    if (batch > 32767 || widest < 2) return BasisRoute::Composed;
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
    const lr_poly *a0 = ops.of(P.a, 0), *a1 = ops.of(P.a, 1), *b0 = ops.of(P.b, 0), *b1 = ops.of(P.b, 1);
    TensorLaunch T;
    T.a0 = a0->d; T.a1 = a1->d; T.b0 = b0->d; T.b1 = b1->d;
    T.a0_stride = a0->stride(); T.a1_stride = a1->stride(); T.b0_stride = b0->stride(); T.b1_stride = b1->stride();
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

extern "C" int lr_ckks_power_basis_schedule(const uint64_t *moduli, int n_moduli, double default_scale, int chebyshev, int c1_level,
                                            double c1_scale, int n_targets, const uint32_t *targets, int capacity, int *n_products,
                                            lr_ckks_basis_product *products, uint64_t *mult, uint64_t *add) {
    return guarded([&]() -> int {
    if (!moduli || !n_products || (n_targets > 0 && !targets) || (capacity > 0 && (!products || !mult || !add))) return refuse_sched("null argument");
    if (n_moduli < 1 || n_targets < 0 || capacity < 0 || c1_level < 0 || c1_level >= n_moduli) return refuse_sched("a count or a level is out of range");
    for (int t = 0; t < n_targets; ++t)
        if (targets[t] == 0 || targets[t] > 65535) return refuse_sched("a target is 0 or above 65535");
    for (int i = 0; i < n_moduli; ++i)
        if (moduli[i] < 3 || !(moduli[i] & 1) || (moduli[i] >> 61)) return refuse_sched("a modulus is even, below 3 or not below 2^61");
    if (!scale_ok(default_scale) || !scale_ok(c1_scale)) return refuse_sched("a scale is not finite and positive");

    Recursion rec;
    for (int t = 0; t < n_targets; ++t) rec.want(targets[t]);
    const int count = (int)rec.order.size();
    if (count > capacity) {
        *n_products = count;      // the one word a refused call writes: the caller sizes its buffers by it and calls again
        return refuse_sched("more products than capacity");
    }

    std::vector<lr_ckks_basis_product> v((size_t)count);
    std::vector<u64> v_mult((size_t)count * n_moduli, 0), v_add((size_t)count * n_moduli, 0);
    struct State { int level, layer; double scale; };
    const auto state = [&](u32 x) { return x == 1 ? State{c1_level, 0, c1_scale} : State{v[rec.at[x]].level_after, v[rec.at[x]].layer, v[rec.at[x]].scale_after}; };
    for (int k = 0; k < count; ++k) {
        lr_ckks_basis_product &P = v[k];
        P.n = rec.order[k];
        P.a = (P.n + 1) >> 1;                                                // uint64(math.Ceil(float64(n) / 2)), :81 / :73
        P.b = P.n >> 1;
        P.c = chebyshev ? P.a - P.b : 0;                                     // :75
        const State A = state(P.a), B = state(P.b);
        P.mul_level = std::min(A.level, B.level);                            // MulRelinNew :1005
        P.layer = 1 + std::max(A.layer, B.layer);
        double scale = A.scale * B.scale;                                    // :1038
        if (!scale_ok(scale)) return refuse_sched("a scale is not finite and positive");
        // Rescale(C[n], ckksContext.scale, C[n]), :938-961: nothing at level 0 (the error return is ignored), else the loop
        int level = P.mul_level;
        P.n_rescales = 0;
        while (level != 0 && scale >= (default_scale * (double)moduli[level]) / 2) {
            scale /= (double)moduli[level];
            --level;
            ++P.n_rescales;
        }
        P.level_after = level;
        P.scale_after = scale;
        P.tail = !chebyshev ? 0 : P.c == 0 ? 2 : 1;
        P.mult_side = 0;
        if (P.tail == 1) {
            // Add(C[n], C[n], C[n]) :92 keeps level and scale; Sub(C[n], C[c], C[n]) :98 with C[c] = C[1]
            int level_after = 0, degree_after = 0, side = 0;
            double scale_after = 0;
            const int rc = lr_ckks_combine_constants(moduli, n_moduli, LR_SUB, 1, level, scale, 1, c1_level, c1_scale, 1, level, scale, LR_COMBINE_OUT_A,
                                                     &level_after, &scale_after, &degree_after, &side, &v_mult[(size_t)k * n_moduli]);
            if (rc != LR_OK) return refuse_sched("a scale ratio is not below 2^63");      // (every other argument is inside its domain)
            P.level_after = level_after;
            P.scale_after = scale_after;
            P.mult_side = side;
        } else if (P.tail == 2) {
            // AddConst(C[n], -1, C[n]) :96: scaleUpExact(-1, scale, q_i), real, so one word for both halves; the scale stays
            for (int i = 0; i <= level; ++i) {
                const Limb m{moduli[i], montgomery_const(moduli[i]), 0, barrett_const(moduli[i])};
                u64 hi;
                half_constants(-1, 0, scale, m, &v_add[(size_t)k * n_moduli + i], &hi);
            }
        }
    }
    // nothing was written so far
    *n_products = count;
    std::copy(v.begin(), v.end(), products);
    std::copy(v_mult.begin(), v_mult.end(), mult);
    std::copy(v_add.begin(), v_add.end(), add);
    return LR_OK;
    });
}

extern "C" int lr_ckks_power_basis(lr_ckks_plan *pl, int n_products, const lr_ckks_basis_product *products, const uint64_t *mult,
                                   const uint64_t *add, int row_words, int c1_level, const lr_poly *c1_c0, const lr_poly *c1_c1,
                                   const lr_poly *evk, lr_poly *const *outs_c0, lr_poly *const *outs_c1) {
    return guarded([&]() -> int {
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
        struct Span { const u64 *lo, *hi; };
        const auto span = [](const lr_poly *p) {
            return Span{p->d, p->d + (long long)(p->batch - 1) * p->stride() + (long long)p->alloc_limbs * (long long)p->N};
        };
        std::vector<Span> spans;
        spans.reserve((size_t)2 * n_products);
        for (int k = 0; k < n_products; ++k) {
            spans.push_back(span(outs_c0[k]));
            spans.push_back(span(outs_c1[k]));
        }
        std::sort(spans.begin(), spans.end(), [](const Span &x, const Span &y) { return x.lo < y.lo; });
        for (size_t i = 1; i < spans.size(); ++i)
            if (spans[i].lo < spans[i - 1].hi) return refuse(LR_ERR_ARG, "two outputs share memory");
        for (const lr_poly *c : {c1_c0, c1_c1}) {
            const Span s = span(c);
            for (const Span &o : spans)
                if (s.lo < o.hi && o.lo < s.hi) return refuse(LR_ERR_ARG, "an output shares memory with C[1]");
        }
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
    const int alpha = pl->dec->alpha, beta = (c1_level + 1 + alpha - 1) / alpha;
    if (evk->N != pl->cQ->h.N || evk->batch < 2 * beta || evk->limbs < pl->cQ->h.L() + pl->cP->h.L())
        return refuse(LR_ERR_SHAPE, "evaluation key: need batch >= 2*beta and |Q|+|P| limbs");
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
