// fbx_tomo_sim_grouped.hip -- simulated tomography with grouped settings (fbx_tomo_simulate_grouped): the settings of a group are
// diagonal in one tensor-product basis and are read off the SAME shots, as the reference's do_tomography(group_tpb_settings=True)
// acquires them -- the ZZ result of a shot is the product of its IZ and ZI results.
//
// A grouping (fbx_grouping) holds, per group, the input state, the basis (the members' non-identity Paulis, Z where no member
// acts) and the members sorted by group, each with its parity mask.  Three launches per call: tomo_poison_kernel (fbx_tomo_sim.hip:
// truth entries and flips), tomog_status_kernel (a wavefront per unit = (item, group): a distribution whose clamped sum is not a
// positive finite number poisons the item) and tomog_sim_kernel (a wavefront per unit), which
//   1. evaluates t_T = tr[P_T .] for the 2^n subsets T of the qubits, lane T each, with tomo_trace_process / tomo_trace_state;
//   2. turns them into the outcome distribution with n shuffle butterflies (Walsh-Hadamard) and n more for the readout flips;
//   3. takes the running sum of the clamped probabilities serially (every lane the same additions: numpy.cumsum restates it) and
//      the 2^n - 1 thresholds floor(c_o / c_last 2^32), kept in LDS;
//   4. counts: lane l draws the Philox blocks l, l + 64, ...; for 4-5 qubits it finds the outcome of each word with an n-step
//      search of the thresholds and increments its PRIVATE counter [outcome][lane] in LDS (conflict-free: the lane is the bank),
//      and the 64 columns are summed at the end (integers, exactly);
//   5. lane j takes member j of the group: the parity sum over the histogram, the integer formulas of fbx_tomo_simulate, and the
//      exact mean with tomo_mean itself (fbx_sim_shared.hpp: the value fbx_tomo_simulate writes, bit for bit).
// The status kernel runs steps 1-3 with the same device function (tomog_distribution, in fbx_tomo_grouping.hpp with the grouping
// object: fbx_tomo_sim_symm.hip evaluates it too), so the two agree on which unit is poisoned.  For 1..3 qubits the
// wavefront form counts in registers instead of LDS (per threshold, the words that reach it), and there is a second work split,
// chosen by the number of units alone: from FBX_TOMOG_LANE_MIN_UNITS units on a LANE takes a unit -- the same sums in the same
// order for the distribution, all the unit's Philox blocks, registers only.  A value depends on (seed, item id, group,
// distribution, shots) only, whichever form ran.  The walk over the Philox blocks, the step from the counts to the histogram
// and the members' formulas are those of fbx_sim_shared.hpp; the wavefront form keeps its own compare (`thi == 0 && tlo <= w` on
// wave-uniform operands), the lane form uses sim_count_word (`live && tlo <= w`) and keeps its own copy of the walk (measured).
#include "fbx_tomo_grouping.hpp"

#ifndef FBX_TOMOG_LANE_MIN_UNITS
#define FBX_TOMOG_LANE_MIN_UNITS 131072          // as FBX_TOMO_LANE_MIN_UNITS: from here on a lane per (item, group) fills the chip
#endif

namespace fbx {

// The same steps by ONE lane for 1..3 qubits, in registers: every sum, difference and product is the one tomog_distribution takes
// (the butterflies pair the same values in the same order), so the two give the same bits.  p: the probabilities, c: the running sums.
template <int NQ>
__device__ __forceinline__ void tomog_distribution_lane(const DesignDev& des, const double* __restrict__ truth,
                                                        const double* __restrict__ flip, int state, int basis,
                                                        double (&p)[1 << NQ], double (&c)[1 << NQ]) {
    constexpr int DD = 1 << NQ;
    p[0] = 1.0;
#pragma unroll
    for (int T = 1; T < DD; ++T) {
        int keep = 0;
#pragma unroll
        for (int t = 0; t < NQ; ++t) if ((T >> t) & 1) keep |= 3 << (2 * t);
        p[T] = des.kind == FBX_KIND_PROCESS ? tomo_trace_process(truth, des.Ct + (size_t)state * des.D, des.D, basis & keep)
                                            : tomo_trace_state(reinterpret_cast<const cplx*>(truth), NQ, basis & keep);
    }
#pragma unroll
    for (int h = 1; h < DD; h <<= 1) {
#pragma unroll
        for (int o = 0; o < DD; ++o) {
            if (o & h) continue;
            const double a = p[o], b = p[o | h];
            p[o] = a + b; p[o | h] = a - b;
        }
    }
#pragma unroll
    for (int o = 0; o < DD; ++o) p[o] *= 1.0 / (double)DD;
    if (flip) {
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            const int q = NQ - 1 - t;
            const double f0 = flip[2 * q], f1 = flip[2 * q + 1];
#pragma unroll
            for (int o = 0; o < DD; ++o) {
                if ((o >> t) & 1) continue;
                const double a = p[o], b = p[o | (1 << t)];
                p[o] = fma(1.0 - f0, a, f1 * b); p[o | (1 << t)] = fma(1.0 - f1, b, f0 * a);
            }
        }
    }
    double run = 0.0;
#pragma unroll
    for (int o = 0; o < DD; ++o) { run += p[o] < 0.0 ? 0.0 : p[o]; c[o] = run; }
}

// status[b] = 1 when a group of item b has a distribution whose clamped sum is not a positive finite number (after tomo_poison_kernel)
__global__ void __launch_bounds__(TOMOG_THREADS)
tomog_status_kernel(DesignDev des, GroupingDev grp, long long B, const double* __restrict__ truth, int truth_len,
                    const double* __restrict__ flips, int* __restrict__ status) {
    __shared__ double pw_all[TOMOG_WAVES][TOMOG_MAX_OUTCOMES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * TOMOG_WAVES + uniform(wave);
    if (u >= B * grp.G) return;
    const long long b = u / grp.G;
    const int g = (int)(u - b * grp.G);
    if (status[b]) return;                                     // (a neighbour's 1 or the poison kernel's: nothing to add)
    double c_mine, c_last;
    (void)tomog_distribution(des, truth + b * truth_len, flips ? flips + b * 2 * des.n : nullptr, grp.gstate[g], grp.gbasis[g], lane,
                             pw_all[wave], &c_mine, &c_last);
    if (lane == 0 && tomog_bad_total(c_last)) status[b] = 1;   // (several wavefronts may store the same 1)
}

// The members first, first + step, ... of group [m0, m1) of a poisoned item, `base` = b * m: (lane, 64) for a wavefront, (0, 1) for a lane
__device__ __forceinline__ void tomog_members_poisoned(const GroupingDev& grp, int m0, int m1, int first, int step, long long base,
                                                       unsigned n_shots, double* __restrict__ expect_out, double* __restrict__ counts_out,
                                                       double* __restrict__ std_err_out, double* __restrict__ exact_out) {
    for (int j = m0 + first; j < m1; j += step) sim_write_poisoned(expect_out, counts_out, std_err_out, exact_out, base + grp.mk[j], n_shots);
}

// ... and of a sampled one: the parity sum over the histogram of the group's d outcomes (LDS words or a lane's registers)
template <class Hist>
__device__ __forceinline__ void tomog_members_sampled(const GroupingDev& grp, int m0, int m1, int first, int step, long long base,
                                                      const Hist& hist, int d, unsigned n_shots, double* __restrict__ expect_out,
                                                      double* __restrict__ counts_out, double* __restrict__ std_err_out) {
    for (int j = m0 + first; j < m1; j += step) {
        const int z = grp.mmask[j];
        unsigned long long k_plus = 0;
#pragma unroll
        for (int o = 0; o < d; ++o) if (!(__popc(o & z) & 1)) k_plus += hist[o];
        sim_write_pm1(expect_out, counts_out, std_err_out, base + grp.mk[j], grp.mcoef[j], k_plus, n_shots);
    }
}

// unit u = (item u / G, group u % G), a wavefront each.  NQ = the number of qubits when it is 1..3: the lanes count in registers,
// per threshold, the words that reach it (2^n - 1 compares against wave-uniform operands and as many adds per word, no LDS);
// NQ = 0: any n, the search and the private LDS counters.  The histogram is the same integers either way.
template <int NQ>
__global__ void __launch_bounds__(TOMOG_THREADS)
tomog_sim_kernel(DesignDev des, GroupingDev grp, long long B, const double* __restrict__ truth, int truth_len,
                 const double* __restrict__ flips, unsigned n_shots, unsigned long long seed, long long first_item,
                 const int* __restrict__ status, double* __restrict__ expect_out, double* __restrict__ counts_out,
                 double* __restrict__ std_err_out, double* __restrict__ exact_out, double* __restrict__ prob_out,
                 uint32_t* __restrict__ hist_out) {
    __shared__ double pw_all[TOMOG_WAVES][TOMOG_MAX_OUTCOMES];
    __shared__ unsigned long long thr_all[TOMOG_WAVES][TOMOG_MAX_OUTCOMES];
    __shared__ uint32_t hist_all[TOMOG_WAVES][TOMOG_MAX_OUTCOMES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * TOMOG_WAVES + uniform(wave);
    if (u >= B * grp.G) return;
    const long long b = u / grp.G;
    const int g = (int)(u - b * grp.G);
    const int n = NQ ? NQ : des.n, d = 1 << n, m0 = grp.mptr[g], m1 = grp.mptr[g + 1];
    const long long cell = (b * grp.G + g) * d + lane;         // of prob_out / hist_out, lanes < d
    if (status[b]) {
        tomog_members_poisoned(grp, m0, m1, lane, 64, b * des.m, n_shots, expect_out, counts_out, std_err_out, exact_out);
        if (lane < d) {
            if (prob_out) prob_out[cell] = __builtin_nan("");
            if (hist_out) hist_out[cell] = 0u;
        }
        return;
    }
    const double* tb = truth + b * truth_len;
    const double* fb = flips ? flips + b * 2 * des.n : nullptr;
    if (exact_out)
        for (int j = m0 + lane; j < m1; j += 64) exact_out[b * des.m + grp.mk[j]] = grp.mcoef[j] * tomo_mean(des, tb, fb, grp.msp[j]);
    const bool sampled = n_shots != 0 && (expect_out || counts_out || std_err_out || hist_out);
    if (!sampled && !prob_out) return;
    double* pw = pw_all[wave];
    double c_mine, c_last;
    const double p = tomog_distribution(des, tb, fb, grp.gstate[g], grp.gbasis[g], lane, pw, &c_mine, &c_last);
    if (prob_out && lane < d) prob_out[cell] = p;
    if (!sampled) return;
    // thresholds: thr[o] = floor(c_o / c_last 2^32), 2^32 for the last outcome (no word reaches it)
    unsigned long long* thr = thr_all[wave];
    uint32_t* hist = hist_all[wave];
    if (lane < d) thr[lane] = lane == d - 1 ? 1ull << 32 : (unsigned long long)(c_mine / c_last * 0x1p32);
    FBX_WAVE_SYNC();
    const unsigned long long gid = (unsigned long long)(first_item + b);
    const uint32_t g0 = (uint32_t)gid, g1 = (uint32_t)(gid >> 32);
    const uint32_t k0 = (uint32_t)seed ^ TOMOG_KEY_TAG, k1 = (uint32_t)(seed >> 32);
    if constexpr (NQ > 0) {
        constexpr int DD = 1 << NQ;
        uint32_t tlo[DD - 1], thi[DD - 1], reach[DD - 1];              // reach[o]: words with thr[o] <= word, i.e. outcome > o
#pragma unroll
        for (int o = 0; o < DD - 1; ++o) {
            const unsigned long long t = thr[o];
            tlo[o] = (uint32_t)uniform((int)(uint32_t)t); thi[o] = (uint32_t)uniform((int)(uint32_t)(t >> 32)); reach[o] = 0u;
        }
        sim_walk(g0, g1, (uint32_t)g, k0, k1, (uint32_t)lane, 64u, n_shots, [&](uint32_t w, uint32_t) {
#pragma unroll
            for (int o = 0; o < DD - 1; ++o) reach[o] += (uint32_t)(thi[o] == 0u && tlo[o] <= w);      // (thi = 1: the threshold is 2^32)
        });
        uint32_t h[DD];
        sim_histogram<DD, false>(reach, n_shots, h);
#pragma unroll
        for (int o = 0; o < DD; ++o) if (lane == o) hist[o] = h[o];
    } else {
        __shared__ uint32_t cnt_all[TOMOG_WAVES][TOMOG_MAX_OUTCOMES * 64];
        uint32_t* cnt = cnt_all[wave];
        for (int o = 0; o < d; ++o) cnt[o * 64 + lane] = 0u;
        FBX_WAVE_SYNC();
        // the outcome of a word = the number of thresholds <= the word: n steps of a search (thr is non-decreasing)
        sim_walk(g0, g1, (uint32_t)g, k0, k1, (uint32_t)lane, 64u, n_shots, [&](uint32_t w, uint32_t) {
            int lo = 0;
            for (int step = d >> 1; step; step >>= 1)
                if (thr[lo + step - 1] <= (unsigned long long)w) lo += step;
            cnt[lo * 64 + lane] += 1u;
        });
        FBX_WAVE_SYNC();
        sim_column_sum(cnt, d, lane, hist);
    }
    FBX_WAVE_SYNC();
    if (hist_out && lane < d) hist_out[cell] = hist[lane];
    FBX_WAVE_SYNC();
    if (!(expect_out || counts_out || std_err_out)) return;
    tomog_members_sampled(grp, m0, m1, lane, 64, b * des.m, hist, d, n_shots, expect_out, counts_out, std_err_out);
}

// the lane-per-unit split (1..3 qubits, from FBX_TOMOG_LANE_MIN_UNITS units on): the status pass ...
template <int NQ>
__global__ void __launch_bounds__(TOMOG_THREADS)
tomog_status_lane_kernel(DesignDev des, GroupingDev grp, long long B, const double* __restrict__ truth, int truth_len,
                         const double* __restrict__ flips, int* __restrict__ status) {
    const long long u = (long long)blockIdx.x * TOMOG_THREADS + threadIdx.x;
    if (u >= B * grp.G) return;
    const long long b = u / grp.G;
    const int g = (int)(u - b * grp.G);
    if (status[b]) return;
    double p[1 << NQ], c[1 << NQ];
    tomog_distribution_lane<NQ>(des, truth + b * truth_len, flips ? flips + b * 2 * NQ : nullptr, grp.gstate[g], grp.gbasis[g], p, c);
    if (tomog_bad_total(c[(1 << NQ) - 1])) status[b] = 1;
}

// ... and the simulation: a lane takes a unit, counts all its shots in registers and writes its members one after the other
template <int NQ>
__global__ void __launch_bounds__(TOMOG_THREADS)
tomog_sim_lane_kernel(DesignDev des, GroupingDev grp, long long B, const double* __restrict__ truth, int truth_len,
                      const double* __restrict__ flips, unsigned n_shots, unsigned long long seed, long long first_item,
                      const int* __restrict__ status, double* __restrict__ expect_out, double* __restrict__ counts_out,
                      double* __restrict__ std_err_out, double* __restrict__ exact_out, double* __restrict__ prob_out,
                      uint32_t* __restrict__ hist_out) {
    constexpr int DD = 1 << NQ;
    const long long u = (long long)blockIdx.x * TOMOG_THREADS + threadIdx.x;
    if (u >= B * grp.G) return;
    const long long b = u / grp.G;
    const int g = (int)(u - b * grp.G);
    const int m0 = grp.mptr[g], m1 = grp.mptr[g + 1];
    const long long cell = (b * grp.G + g) * DD;
    if (status[b]) {
        tomog_members_poisoned(grp, m0, m1, 0, 1, b * des.m, n_shots, expect_out, counts_out, std_err_out, exact_out);
#pragma unroll
        for (int o = 0; o < DD; ++o) {
            if (prob_out) prob_out[cell + o] = __builtin_nan("");
            if (hist_out) hist_out[cell + o] = 0u;
        }
        return;
    }
    const double* tb = truth + b * truth_len;
    const double* fb = flips ? flips + b * 2 * NQ : nullptr;
    if (exact_out)
        for (int j = m0; j < m1; ++j) exact_out[b * des.m + grp.mk[j]] = grp.mcoef[j] * tomo_mean(des, tb, fb, grp.msp[j]);
    const bool sampled = n_shots != 0 && (expect_out || counts_out || std_err_out || hist_out);
    if (!sampled && !prob_out) return;
    double p[DD], c[DD];
    tomog_distribution_lane<NQ>(des, tb, fb, grp.gstate[g], grp.gbasis[g], p, c);
    if (prob_out) {
#pragma unroll
        for (int o = 0; o < DD; ++o) prob_out[cell + o] = p[o];
    }
    if (!sampled) return;
    uint32_t tlo[DD - 1], reach[DD - 1];
    bool live[DD - 1];
    sim_thresholds<DD>(c, tlo, live, reach);
    const unsigned long long gid = (unsigned long long)(first_item + b);
    const uint32_t g0 = (uint32_t)gid, g1 = (uint32_t)(gid >> 32);
    const uint32_t k0 = (uint32_t)seed ^ TOMOG_KEY_TAG, k1 = (uint32_t)(seed >> 32);
    // This kernel keeps the walk of sim_walk(.., 0, 1, ..) spelled out: through the helper the loop is the same instructions in
    // other registers and 0.9 % slower at 65536 x 324 units.
    const uint32_t full = n_shots >> 2, tail = n_shots & 3u;
    auto count_word = [&](uint32_t w) { (void)sim_count_word<DD>(w, tlo, live, reach); };
    for (uint32_t j = 0; j < full; ++j) {
        uint32_t x[4] = {g0, g1, (uint32_t)g, j};
        philox4x32_10(x, k0, k1);
        count_word(x[0]); count_word(x[1]); count_word(x[2]); count_word(x[3]);
    }
    if (tail) {
        uint32_t x[4] = {g0, g1, (uint32_t)g, full};
        philox4x32_10(x, k0, k1);
        count_word(x[0]);
        if (tail > 1) count_word(x[1]);
        if (tail > 2) count_word(x[2]);
    }
    uint32_t hist[DD];
    sim_histogram<DD, true>(reach, n_shots, hist);
    if (hist_out) {
#pragma unroll
        for (int o = 0; o < DD; ++o) hist_out[cell + o] = hist[o];
    }
    if (!(expect_out || counts_out || std_err_out)) return;
    tomog_members_sampled(grp, m0, m1, 0, 1, b * des.m, hist, DD, n_shots, expect_out, counts_out, std_err_out);
}

static int tomog_check(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const void* truth, int64_t n_shots,
                       int64_t first_item, const void* expect, const void* counts, const void* std_err, const void* exact,
                       const void* prob, const void* hist) {
    const char* who = "fbx_tomo_simulate_grouped";
    FBX_TRY(sim_check_batch(who, B, n_shots, first_item));
    FBX_REQUIRE(truth != nullptr, "fbx_tomo_simulate_grouped: NULL truth");
    FBX_REQUIRE(expect || counts || std_err || exact || prob || hist, "fbx_tomo_simulate_grouped: every output is NULL");
    FBX_REQUIRE(n_shots > 0 || !(expect || counts || std_err || hist),
                "fbx_tomo_simulate_grouped: n_shots == 0 gives exact_out and prob_out only (the sampled outputs must be NULL)");
    FBX_TRY(check_design(design, who));
    return check_grouping(grouping, design, who);
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_grouping_create(const fbx_design* design, int n_groups, const int32_t* group_of, fbx_grouping** out) {
    FBX_REQUIRE(out != nullptr, "fbx_grouping_create: NULL out");
    *out = nullptr;
    FBX_TRY(check_design(design, "fbx_grouping_create"));
    FBX_REQUIRE(group_of != nullptr, "fbx_grouping_create: NULL group_of");
    const int m = design->dev.m, n = design->dev.n, G = n_groups;
    FBX_REQUIRE(G >= 1 && G <= m, "fbx_grouping_create: n_groups must be in [1, m]");
    // the settings in the caller's order: (state, Pauli) and coefficient
    std::vector<uint32_t> sp(m);
    std::vector<double> coef(m);
    for (int j = 0; j < m; ++j) { sp[design->order_host[j]] = design->sp_host[j]; coef[design->order_host[j]] = design->coef_host[j]; }
    std::vector<int> mptr(G + 1, 0), gstate(G, -1), gbasis(G, 0);
    for (int k = 0; k < m; ++k) {
        FBX_REQUIRE(group_of[k] >= 0 && group_of[k] < G, "fbx_grouping_create: a group id is outside [0, n_groups)");
        mptr[group_of[k] + 1]++;
    }
    for (int g = 0; g < G; ++g) {
        FBX_REQUIRE(mptr[g + 1] > 0, "fbx_grouping_create: a group has no member");
        mptr[g + 1] += mptr[g];
    }
    std::vector<int> fill(mptr.begin(), mptr.end() - 1), mk(m), mmask(m);
    std::vector<uint32_t> msp(m);
    std::vector<double> mcoef(m);
    for (int k = 0; k < m; ++k) {
        const int g = group_of[k], s = (int)(sp[k] >> 16), pidx = (int)(sp[k] & 0xFFFFu);
        if (gstate[g] < 0) gstate[g] = s;
        FBX_REQUIRE(gstate[g] == s, "fbx_grouping_create: the members of a group have different input states");
        int mask = 0;
        for (int t = 0; t < n; ++t) {
            const int code = (pidx >> (2 * t)) & 3, have = (gbasis[g] >> (2 * t)) & 3;
            if (!code) continue;
            mask |= 1 << t;
            FBX_REQUIRE(have == 0 || have == code, "fbx_grouping_create: the members of a group are not diagonal in one tensor-product basis");
            gbasis[g] |= code << (2 * t);
        }
        const int j = fill[g]++;
        mk[j] = k; msp[j] = sp[k]; mmask[j] = mask; mcoef[j] = coef[k];
    }
    for (int g = 0; g < G; ++g)
        for (int t = 0; t < n; ++t) if (!((gbasis[g] >> (2 * t)) & 3)) gbasis[g] |= 3 << (2 * t);     // Z where no member acts
    FBX_TRY(ensure_device());
    // one slab: mcoef | gstate | gbasis | mptr | mk | msp | mmask
    const size_t oCoef = 0, oState = oCoef + sizeof(double) * m, oBasis = oState + sizeof(int) * G, oPtr = oBasis + sizeof(int) * G;
    const size_t oK = oPtr + sizeof(int) * (G + 1), oSp = oK + sizeof(int) * m, oMask = oSp + sizeof(uint32_t) * m;
    const size_t total = oMask + sizeof(int) * m;
    std::vector<char> host(total);
    memcpy(&host[oCoef], mcoef.data(), sizeof(double) * m);
    memcpy(&host[oState], gstate.data(), sizeof(int) * G);
    memcpy(&host[oBasis], gbasis.data(), sizeof(int) * G);
    memcpy(&host[oPtr], mptr.data(), sizeof(int) * (G + 1));
    memcpy(&host[oK], mk.data(), sizeof(int) * m);
    memcpy(&host[oSp], msp.data(), sizeof(uint32_t) * m);
    memcpy(&host[oMask], mmask.data(), sizeof(int) * m);
    auto* grp = new fbx_grouping();
    hipError_t e = hipMalloc(&grp->slab, total);
    if (e != hipSuccess) { delete grp; return hip_fail(e, "hipMalloc(grouping)", __FILE__, __LINE__); }
    e = hipMemcpy(grp->slab, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(grp->slab); delete grp; return hip_fail(e, "hipMemcpy(grouping)", __FILE__, __LINE__); }
    const char* base = (const char*)grp->slab;
    grp->dev.G = G;
    grp->dev.mcoef = (const double*)(base + oCoef);
    grp->dev.gstate = (const int*)(base + oState);
    grp->dev.gbasis = (const int*)(base + oBasis);
    grp->dev.mptr = (const int*)(base + oPtr);
    grp->dev.mk = (const int*)(base + oK);
    grp->dev.msp = (const uint32_t*)(base + oSp);
    grp->dev.mmask = (const int*)(base + oMask);
    grp->design = design; grp->device = current_device(); grp->epoch = device_epoch();
    grp->gunion_host.assign(G, 0);
    for (int g = 0; g < G; ++g)
        for (int j = mptr[g]; j < mptr[g + 1]; ++j) grp->gunion_host[g] |= mmask[j];
    *out = grp;
    return FBX_OK;
}

int fbx_grouping_destroy(fbx_grouping* grouping) {
    if (!grouping) return FBX_OK;
    if (grouping->slab) (void)hipFree(grouping->slab);
    delete grouping;
    return FBX_OK;
}

int fbx_tomo_simulate_grouped_dev(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const double* d_truth,
                                  int64_t n_shots, const double* d_readout_flip, uint64_t seed, int64_t first_item,
                                  double* d_expect_out, double* d_counts_out, double* d_std_err_out, double* d_exact_out,
                                  double* d_prob_out, uint32_t* d_hist_out, int32_t* d_status_out) {
    FBX_TRY(tomog_check(design, grouping, B, d_truth, n_shots, first_item, d_expect_out, d_counts_out, d_std_err_out, d_exact_out,
                        d_prob_out, d_hist_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const DesignDev& des = design->dev;
    const GroupingDev& grp = grouping->dev;
    const int truth_len = tomo_truth_len(des);
    StatusBuf status_buf;
    FBX_TRY(status_buf.take(d_status_out, B));
    int32_t* status = status_buf.p;
    FBX_TRY(tomo_poison_launch(B, truth_len, 2 * des.n, d_truth, d_readout_flip, status));
    const int64_t units = B * grp.G;
    const bool lane = des.n <= 3 && units >= FBX_TOMOG_LANE_MIN_UNITS;       // (4 and 5 qubits: the wavefront form at any size)
    const int64_t per_block = lane ? TOMOG_THREADS : TOMOG_WAVES, blocks = (units + per_block - 1) / per_block;
    FBX_REQUIRE(blocks < ((int64_t)1 << 31), "fbx_tomo_simulate_grouped: B * n_groups is beyond one launch; cut the batch with first_item");
    auto launch_status = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(TOMOG_THREADS), 0, stream(), des, grp, (long long)B, d_truth,
                           truth_len, d_readout_flip, status);
    };
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(TOMOG_THREADS), 0, stream(), des, grp, (long long)B, d_truth,
                           truth_len, d_readout_flip, (unsigned)n_shots, (unsigned long long)seed, (long long)first_item,
                           (const int*)status, d_expect_out, d_counts_out, d_std_err_out, d_exact_out, d_prob_out, d_hist_out);
    };
    if (lane) {
        if (des.n == 1) launch_status(tomog_status_lane_kernel<1>);
        else if (des.n == 2) launch_status(tomog_status_lane_kernel<2>);
        else launch_status(tomog_status_lane_kernel<3>);
        FBX_HIP(hipGetLastError());
        if (des.n == 1) launch(tomog_sim_lane_kernel<1>);
        else if (des.n == 2) launch(tomog_sim_lane_kernel<2>);
        else launch(tomog_sim_lane_kernel<3>);
    } else {
        launch_status(tomog_status_kernel);
        FBX_HIP(hipGetLastError());
        if (des.n == 1) launch(tomog_sim_kernel<1>);
        else if (des.n == 2) launch(tomog_sim_kernel<2>);
        else if (des.n == 3) launch(tomog_sim_kernel<3>);
        else launch(tomog_sim_kernel<0>);
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_tomo_simulate_grouped(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const double* truth,
                              int64_t n_shots, const double* readout_flip, uint64_t seed, int64_t first_item, double* expect_out,
                              double* counts_out, double* std_err_out, double* exact_out, double* prob_out, uint32_t* hist_out,
                              int32_t* status_out) {
    FBX_TRY(tomog_check(design, grouping, B, truth, n_shots, first_item, expect_out, counts_out, std_err_out, exact_out, prob_out,
                        hist_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t n = (size_t)B, m = (size_t)design->dev.m, cells = (size_t)grouping->dev.G << design->dev.n;
    HostIO io; SimOut o; double *dt, *df = nullptr, *dp; uint32_t* dh;
    FBX_TRY(io.in(truth, n * (size_t)tomo_truth_len(design->dev), &dt));
    if (readout_flip) FBX_TRY(io.in(readout_flip, n * 2 * (size_t)design->dev.n, &df));
    FBX_TRY(o.stage(io, n, n * m, expect_out, counts_out, std_err_out, exact_out, status_out));
    FBX_TRY(io.out_opt(prob_out, n * cells, &dp));
    FBX_TRY(io.out_opt(hist_out, n * cells, &dh));
    FBX_TRY(fbx_tomo_simulate_grouped_dev(design, grouping, B, dt, n_shots, df, seed, first_item, o.expect, o.counts, o.std_err, o.exact,
                                          dp, dh, o.status));
    return io.finish();
}

}  // fbx C ABI
