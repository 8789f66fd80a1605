// fbx_tomo_sim_symm.hip -- simulated tomography under a JOINT readout confusion matrix, with the reference's two defaults of
// do_tomography: exhaustive readout symmetrization (symm_type = -1) and the calibration of every observable on its +1 eigenstate
// (fbx_tomo_simulate_symmetrized, fbx_tomo_simulate_calibration; the contract is in include/fbx.h).
//
// One kernel body serves both calls.  A unit is (item, group) for the measurement and (item, calibration) for the calibration,
// a wavefront each; the calibration is the measurement of the distribution "outcome 0 with certainty" with one member whose mask
// is the calibration's.  Per unit:
//   1. the item's confusion matrix goes to LDS (every entry is looked at: one outside [0, 1] poisons the item);
//   2. the ideal distribution p of the group with tomog_distribution (fbx_tomo_grouping.hpp, no flips), kept in LDS;
//   3. the patterns: the submasks f of U (the union of the members' masks), 64 / 2^n of them per pass, lane (slot, r) takes
//      q_f(r) = sum_o p(o) C[o ^ f][r ^ f], one fma per term in ascending o; the running clamped sum of a pattern serially, every
//      lane the same additions; the thresholds as 32-bit words plus, per pattern, how many of them are below 2^32 (they are
//      non-decreasing, so those form a prefix);
//   4. counting: the (pattern, Philox block) pairs are flattened over the lanes -- a pattern of a hundred shots has fewer blocks
//      than the wavefront has lanes -- and every word increments the lane's PRIVATE counter [outcome][lane] in LDS (the lane is
//      the bank); the 64 columns are summed at the end.  The histogram is the integer sum over the patterns;
//   5. members: the integer formulas of fbx_tomo_simulate_grouped on the merged histogram with N = s x patterns, and the exact
//      mean from the mean of the q_f.
// The status pass runs steps 1-3 with the same code, so the two agree on which item is poisoned.  LDS is sized by 2^n at the
// launch (two wavefronts per workgroup: 43.5 KB at five qubits, 1.6 KB at two).
#include "fbx_tomo_grouping.hpp"

namespace fbx {

constexpr int TOMS_WAVES = 2;
constexpr int TOMS_THREADS = TOMS_WAVES * 64;
constexpr uint32_t TOMS_KEY_TAG = 0x544F4D53u;      // "TOMS": the shots of fbx_tomo_simulate_symmetrized
constexpr uint32_t TOMC_KEY_TAG = 0x544F4D43u;      // "TOMC": the shots of fbx_tomo_simulate_calibration
constexpr int64_t TOMS_MAX_PER_PATTERN = (int64_t)1 << 29;      // (f << 27) | (shot >> 2) is one counter word

// per-wavefront LDS, in bytes: doubles conf [d][d], pw [d], qrow [64], qsum [d]; words thr [d][d], nlive [d], cnt [d][64], hist [d]
static size_t toms_lds_per_wave(int n) {
    const size_t d = (size_t)1 << n;
    return sizeof(double) * (d * d + d + 64 + d) + sizeof(uint32_t) * (d * d + d + 64 * d + d);
}

// bit i of `idx` goes to the i-th set bit of `mask` (ascending): the idx-th submask of `mask` in ascending order
__device__ __forceinline__ int toms_deposit(int idx, int mask) {
    int f = 0;
    for (int t = 0, i = 0; t < 5; ++t)
        if ((mask >> t) & 1) { f |= ((idx >> i) & 1) << t; ++i; }
    return f;
}

struct SymmOut {
    double* expect;       // [B][m]; the calibration: cal_mean [B][n_cal]
    double* counts;
    double* std_err;      // the calibration: cal_var
    double* exact;
    double* prob;         // [B][G][d][d], the measurement only
    uint32_t* hist;       // [B][G][d], the measurement only
};

// CAL: units are (item, calibration); STATUS: steps 1-3 only, status[b] = 1 for a poisoned item
template <bool CAL, bool STATUS>
__global__ void __launch_bounds__(TOMS_THREADS)
toms_kernel(DesignDev des, GroupingDev grp, const int* __restrict__ cal_mask, int n_cal, long long B,
            const double* __restrict__ truth, int truth_len, const double* __restrict__ confusion, int symm, unsigned n_shots,
            unsigned long long seed, long long first_item, int* __restrict__ status, SymmOut out) {
    extern __shared__ double toms_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int G = CAL ? n_cal : grp.G;
    const long long u = (long long)blockIdx.x * TOMS_WAVES + uniform(wave);
    if (u >= B * G) return;
    const long long b = u / G;
    const int g = (int)(u - b * G);
    const int n = des.n, d = 1 << n, dd = d * d;
    // the wavefront's LDS
    const size_t n_doubles = (size_t)dd + d + 64 + d, n_words = (size_t)dd + d + 64 * d + d;
    double* conf = toms_lds + (size_t)wave * (n_doubles + n_words / 2);      // (n_words is even)
    double* pw = conf + dd;
    double* qrow = pw + d;
    double* qsum = qrow + 64;
    uint32_t* thr = reinterpret_cast<uint32_t*>(qsum + d);
    uint32_t* nlive = thr + dd;
    uint32_t* cnt = nlive + d;
    uint32_t* hist = cnt + 64 * d;

    // the patterns of the unit: the submasks of U, or 0 alone
    int U = 0, m0 = 0, m1 = 0;
    if constexpr (CAL) U = cal_mask[g];
    else {
        m0 = grp.mptr[g]; m1 = grp.mptr[g + 1];
        for (int j = m0; j < m1; ++j) U |= grp.mmask[j];
    }
    const int P = symm == -1 ? 1 << __popc(U) : 1;
    const unsigned s = n_shots / (unsigned)P;
    const unsigned long long N = (unsigned long long)s * (unsigned)P;
    const double nd = (double)N;
    const long long cell = (b * G + g) * d;                     // of hist; x d for prob

    if constexpr (STATUS) {
        if (status[b]) return;                                  // (a neighbour's 1 or the truth's: nothing to add)
    } else if (status[b]) {
        if constexpr (CAL) {
            if (lane == 0) sim_write_poisoned(out.expect, out.counts, out.std_err, out.exact, b * n_cal + g, N);
        } else {
            for (int j = m0 + lane; j < m1; j += 64)
                sim_write_poisoned(out.expect, out.counts, out.std_err, out.exact, b * des.m + grp.mk[j], N);
            if (out.prob) for (int i = lane; i < dd; i += 64) out.prob[cell * d + i] = __builtin_nan("");
            if (out.hist && lane < d) out.hist[cell + lane] = 0u;
        }
        return;
    }
    const bool sampled = !STATUS && s != 0 && (out.expect || out.counts || out.std_err || out.hist);
    if (!STATUS && !sampled && !out.prob && !out.exact) return;

    // 1. the confusion matrix
    const double* cb = confusion + b * dd;
    bool bad = false;
    for (int i = lane; i < dd; i += 64) {
        const double v = cb[i];
        conf[i] = v;
        if (tomo_bad_probability(v)) bad = true;
    }
    if constexpr (STATUS) {
        if (__ballot(bad)) { if (lane == 0) status[b] = 1; return; }
    }
    // 2. the ideal distribution
    if constexpr (CAL) {
        FBX_WAVE_SYNC();
        if (lane < d) pw[lane] = lane == 0 ? 1.0 : 0.0;         // the +1 eigenstate on the support, |0> elsewhere: all bits 0
    } else {
        double c_mine, c_last;
        (void)tomog_distribution(des, truth + b * truth_len, nullptr, grp.gstate[g], grp.gbasis[g], lane, pw, &c_mine, &c_last);
    }
    if (lane < d) qsum[lane] = 0.0;
    FBX_WAVE_SYNC();
    if (!STATUS && out.prob)                                     // a zero row for a mask that is not a pattern of the unit
        for (int i = lane; i < dd; i += 64) {
            const int f = i >> n;
            if (symm == -1 ? (f & ~U) != 0 : f != 0) out.prob[cell * d + i] = 0.0;
        }
    // 3. the patterns, 64 / d per pass
    const int slots = 64 >> n, slot = lane >> n, r = lane & (d - 1);
    const unsigned long long dmask = d == 64 ? ~0ull : (1ull << d) - 1ull;
    for (int pi0 = 0; pi0 < P; pi0 += slots) {
        const int pi = pi0 + slot;
        const bool valid = pi < P;
        const int f = valid ? toms_deposit(pi, U) : 0;
        double q = 0.0;
        for (int o = 0; o < d; ++o) q = fma(pw[o], conf[((o ^ f) << n) + (r ^ f)], q);
        FBX_WAVE_SYNC();
        qrow[lane] = q;
        FBX_WAVE_SYNC();
        double c = 0.0, mine = 0.0;
        for (int o = 0; o < d; ++o) {                            // one addition per outcome, in outcome order
            const double v = qrow[(slot << n) + o];
            c += v < 0.0 ? 0.0 : v;
            if (o == r) mine = c;
        }
        if (valid && tomog_bad_total(c)) bad = true;
        if constexpr (!STATUS) {
            if (out.prob && valid) out.prob[(cell + f) * d + r] = q;
            unsigned long long t = 0;
            if (valid && r < d - 1) t = (unsigned long long)(mine / c * 0x1p32);
            const bool live = valid && r < d - 1 && t < (1ull << 32);
            const unsigned long long bal = __ballot(live);
            if (valid) {
                if (r < d - 1) thr[pi * d + r] = (uint32_t)t;
                if (r == 0) nlive[pi] = (uint32_t)__popcll((bal >> (slot << n)) & dmask);
            }
            if (lane < d)                                         // the sum of the q_f, in ascending pattern order
                for (int sl = 0; sl < slots && pi0 + sl < P; ++sl) qsum[lane] += qrow[(sl << n) + lane];
        }
    }
    if constexpr (STATUS) {
        if (__ballot(bad) && lane == 0) status[b] = 1;           // (several wavefronts may store the same 1)
        return;
    }
    FBX_WAVE_SYNC();
    // the exact means: coef sum_r (-1)^{|r & z|} qbar(r), r ascending; qbar = the sum over the patterns / their number (a power of two)
    const double inv_p = 1.0 / (double)P;
    auto exact_of = [&](int z) {
        double acc = 0.0;
        for (int o = 0; o < d; ++o) { const double v = qsum[o] * inv_p; acc += (__popc(o & z) & 1) ? -v : v; }
        return acc;
    };
    if (out.exact) {
        if constexpr (CAL) { if (lane == 0) out.exact[b * n_cal + g] = exact_of(U); }
        else for (int j = m0 + lane; j < m1; j += 64) out.exact[b * des.m + grp.mk[j]] = grp.mcoef[j] * exact_of(grp.mmask[j]);
    }
    if (!sampled) return;
    // 4. the shots: item i of the flattened list = (pattern i / nb, block i % nb), nb blocks of four words per pattern
    for (int o = 0; o < d; ++o) cnt[o * 64 + lane] = 0u;
    FBX_WAVE_SYNC();
    const unsigned long long gid = (unsigned long long)(first_item + b);
    const uint32_t g0 = (uint32_t)gid, g1 = (uint32_t)(gid >> 32);
    const uint32_t k0 = (uint32_t)seed ^ (CAL ? TOMC_KEY_TAG : TOMS_KEY_TAG), k1 = (uint32_t)(seed >> 32);
    const uint32_t nb = (s + 3u) >> 2, tail = s & 3u;
    uint32_t pi = (uint32_t)lane / nb, j = (uint32_t)lane - pi * nb;
    while (pi < (uint32_t)P) {
        const uint32_t f = (uint32_t)toms_deposit((int)pi, U);
        const uint32_t* tp = thr + pi * d;
        const int nl = (int)nlive[pi];
        uint32_t x[4] = {g0, g1, (uint32_t)g, (f << 27) | j};
        philox4x32_10(x, k0, k1);
        const uint32_t words = (tail && j == nb - 1u) ? tail : 4u;
        // the outcome of a word = the number of thresholds <= the word: n steps of a search (thr is non-decreasing)
        for (uint32_t w = 0; w < words; ++w) {
            const uint32_t word = w == 0 ? x[0] : w == 1 ? x[1] : w == 2 ? x[2] : x[3];
            int lo = 0;
            for (int step = d >> 1; step; step >>= 1) {
                const int at = lo + step - 1;
                if (at < nl && tp[at] <= word) lo += step;
            }
            cnt[lo * 64 + lane] += 1u;
        }
        j += 64u;
        if (j >= nb) { const uint32_t adv = j / nb; pi += adv; j -= adv * nb; }
    }
    FBX_WAVE_SYNC();
    sim_column_sum(cnt, d, lane, hist);
    FBX_WAVE_SYNC();
    if (!CAL && out.hist && lane < d) out.hist[cell + lane] = hist[lane];
    // 5. the members
    auto k_plus_of = [&](int z) {
        unsigned long long k = 0;
        for (int o = 0; o < d; ++o) if (!(__popc(o & z) & 1)) k += hist[o];
        return k;
    };
    if constexpr (CAL) {
        if (lane == 0) {
            const unsigned long long k_plus = k_plus_of(U), k_minus = N - k_plus;
            const long long o = b * n_cal + g;
            if (out.expect) out.expect[o] = (double)((long long)k_plus - (long long)k_minus) / nd;
            if (out.counts) out.counts[o] = nd;
            if (out.std_err) out.std_err[o] = (double)(k_plus * k_minus) * 4.0 / nd / nd / nd;      // var / N of the +-1 values
        }
    } else {
        if (!(out.expect || out.counts || out.std_err)) return;
        for (int jm = m0 + lane; jm < m1; jm += 64)
            sim_write_pm1(out.expect, out.counts, out.std_err, b * des.m + grp.mk[jm], grp.mcoef[jm], k_plus_of(grp.mmask[jm]), N);
    }
}

// the calibrations of a design: its distinct non-identity Pauli indices in order of first appearance in the caller's setting order
static int toms_calibrations(const fbx_design* design) {
    std::lock_guard<std::mutex> lock(design->replica_mu);
    if (design->cal_ready) return FBX_OK;
    const int m = design->dev.m, n = design->dev.n;
    std::vector<int> pauli_of(m), index(m, -1), list, masks;
    for (int j = 0; j < m; ++j) pauli_of[design->order_host[j]] = (int)(design->sp_host[j] & 0xFFFFu);
    std::map<int, int> seen;
    for (int k = 0; k < m; ++k) {
        if (pauli_of[k] == 0) continue;
        auto it = seen.find(pauli_of[k]);
        if (it == seen.end()) {
            it = seen.emplace(pauli_of[k], (int)list.size()).first;
            list.push_back(pauli_of[k]);
            int mask = 0;
            for (int t = 0; t < n; ++t) if ((pauli_of[k] >> (2 * t)) & 3) mask |= 1 << t;
            masks.push_back(mask);
        }
        index[k] = it->second;
    }
    if (!masks.empty()) {
        void* slab = nullptr;
        FBX_HIP(hipMalloc(&slab, sizeof(int) * masks.size()));
        const hipError_t e = hipMemcpy(slab, masks.data(), sizeof(int) * masks.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(slab); return hip_fail(e, "hipMemcpy(calibration masks)", __FILE__, __LINE__); }
        design->cal_slab = slab;
    }
    design->cal_pauli_host = list; design->cal_index_host = index; design->cal_ready = true;
    return FBX_OK;
}

// the arguments both calls share; n_shots is the total of a unit
static int toms_check_common(const char* who, const fbx_design* design, int64_t B, const void* confusion, int symm_type,
                             int64_t n_shots, int64_t first_item) {
    const std::string w(who);
    FBX_TRY(sim_check_batch(who, B, n_shots, first_item, true));
    FBX_REQUIRE(confusion != nullptr, w + ": NULL confusion");
    FBX_REQUIRE(symm_type >= -1 && symm_type <= 3, w + ": symm_type must be -1 (exhaustive), 0 (none) or an orthogonal-array strength 1..3");
    FBX_TRY(check_design(design, who));
    if (symm_type >= 1) {
        set_error(w + ": orthogonal-array symmetrization (symm_type 1, 2, 3) is not implemented; use -1 (exhaustive) or 0 (none)");
        return FBX_ERR_UNSUPPORTED;
    }
    return FBX_OK;
}

// the shots of a pattern, s = floor(n_shots / patterns), must be in [1, 2^29) for every unit; masks: the U of every unit
static int toms_check_shots(const char* who, const std::vector<int>& masks, int symm_type, int64_t n_shots) {
    const std::string w(who);
    for (int U : masks) {
        const int64_t patterns = symm_type == -1 ? (int64_t)1 << __builtin_popcount((unsigned)U) : 1, s = n_shots / patterns;
        FBX_REQUIRE(s >= 1, w + ": fewer shots than flip patterns for a unit (shots per pattern = floor(shots / patterns) would be 0)");
        FBX_REQUIRE(s < TOMS_MAX_PER_PATTERN, w + ": 2^29 or more shots per flip pattern");
    }
    return FBX_OK;
}

static int toms_check(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const void* truth, const void* confusion,
                      int symm_type, int64_t n_shots, int64_t first_item, const void* expect, const void* counts, const void* std_err,
                      const void* exact, const void* prob, const void* hist) {
    const char* who = "fbx_tomo_simulate_symmetrized";
    FBX_REQUIRE(truth != nullptr, "fbx_tomo_simulate_symmetrized: NULL truth");
    FBX_TRY(toms_check_common(who, design, B, confusion, symm_type, n_shots, first_item));
    FBX_REQUIRE(expect || counts || std_err || exact || prob || hist, "fbx_tomo_simulate_symmetrized: every output is NULL");
    FBX_REQUIRE(n_shots > 0 || !(expect || counts || std_err || hist),
                "fbx_tomo_simulate_symmetrized: n_shots == 0 gives exact_out and prob_out only (the sampled outputs must be NULL)");
    FBX_TRY(check_grouping(grouping, design, who));
    if (n_shots > 0) FBX_TRY(toms_check_shots(who, grouping->gunion_host, symm_type, n_shots));
    return FBX_OK;
}

static int tomc_check(const fbx_design* design, int64_t B, const void* confusion, int symm_type, int64_t cal_shots,
                      int64_t first_item, const void* mean, const void* var, const void* exact, const void* counts) {
    const char* who = "fbx_tomo_simulate_calibration";
    FBX_TRY(toms_check_common(who, design, B, confusion, symm_type, cal_shots, first_item));
    FBX_REQUIRE(mean || var || exact || counts, "fbx_tomo_simulate_calibration: every output is NULL");
    FBX_REQUIRE(cal_shots > 0 || !(mean || var || counts),
                "fbx_tomo_simulate_calibration: cal_shots == 0 gives cal_exact_out only (the sampled outputs must be NULL)");
    if (cal_shots > 0) {
        const int n = design->dev.n;
        std::vector<int> masks;
        for (int j = 0; j < design->dev.m; ++j) {
            int mask = 0;
            for (int t = 0; t < n; ++t) if ((design->sp_host[j] >> (2 * t)) & 3u) mask |= 1 << t;
            if (mask) masks.push_back(mask);
        }
        FBX_TRY(toms_check_shots(who, masks, symm_type, cal_shots));
    }
    return FBX_OK;
}

template <bool CAL>
static int toms_launch(const fbx_design* design, const GroupingDev& grp, const int* d_cal_mask, int n_cal, int64_t B,
                       const double* d_truth, const double* d_confusion, int symm_type, int64_t n_shots, uint64_t seed,
                       int64_t first_item, const SymmOut& out, int32_t* d_status_out, const char* who) {
    const DesignDev& des = design->dev;
    const int truth_len = CAL ? 0 : tomo_truth_len(des);
    StatusBuf status_buf;
    FBX_TRY(status_buf.take(d_status_out, B));
    int32_t* status = status_buf.p;
    if (CAL) FBX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)B, stream()));
    else FBX_TRY(tomo_poison_launch(B, truth_len, 0, d_truth, nullptr, status));
    const int64_t units = B * (CAL ? n_cal : grp.G), blocks = (units + TOMS_WAVES - 1) / TOMS_WAVES;
    FBX_REQUIRE(blocks < ((int64_t)1 << 31), std::string(who) + ": the number of units is beyond one launch; cut the batch with first_item");
    if (units == 0) return FBX_OK;
    const size_t lds = TOMS_WAVES * toms_lds_per_wave(des.n);
    FBX_TRY(launch_lds(toms_kernel<CAL, true>, dim3((unsigned)blocks), dim3(TOMS_THREADS), lds, des, grp, d_cal_mask, n_cal,
                       (long long)B, d_truth, truth_len, d_confusion, symm_type, (unsigned)n_shots, (unsigned long long)seed,
                       (long long)first_item, (int*)status, out));
    FBX_TRY(launch_lds(toms_kernel<CAL, false>, dim3((unsigned)blocks), dim3(TOMS_THREADS), lds, des, grp, d_cal_mask, n_cal,
                       (long long)B, d_truth, truth_len, d_confusion, symm_type, (unsigned)n_shots, (unsigned long long)seed,
                       (long long)first_item, (int*)status, out));
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_tomo_calibration_list(const fbx_design* design, int32_t* n_cal_out, int32_t* cal_pauli_out, int32_t* cal_index_out) {
    FBX_TRY(check_design(design, "fbx_tomo_calibration_list"));
    FBX_REQUIRE(n_cal_out != nullptr, "fbx_tomo_calibration_list: NULL n_cal_out");
    FBX_TRY(ensure_device());
    FBX_TRY(toms_calibrations(design));
    *n_cal_out = (int32_t)design->cal_pauli_host.size();
    if (cal_pauli_out) for (size_t c = 0; c < design->cal_pauli_host.size(); ++c) cal_pauli_out[c] = design->cal_pauli_host[c];
    if (cal_index_out) for (int k = 0; k < design->dev.m; ++k) cal_index_out[k] = design->cal_index_host[k];
    return FBX_OK;
}

int fbx_tomo_simulate_symmetrized_dev(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const double* d_truth,
                                      const double* d_confusion, int symm_type, int64_t n_shots, uint64_t seed, int64_t first_item,
                                      double* d_expect_out, double* d_counts_out, double* d_std_err_out, double* d_exact_out,
                                      double* d_prob_out, uint32_t* d_hist_out, int32_t* d_status_out) {
    FBX_TRY(toms_check(design, grouping, B, d_truth, d_confusion, symm_type, n_shots, first_item, d_expect_out, d_counts_out,
                       d_std_err_out, d_exact_out, d_prob_out, d_hist_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const SymmOut out{d_expect_out, d_counts_out, d_std_err_out, d_exact_out, d_prob_out, d_hist_out};
    return toms_launch<false>(design, grouping->dev, nullptr, 0, B, d_truth, d_confusion, symm_type, n_shots, seed, first_item, out,
                              d_status_out, "fbx_tomo_simulate_symmetrized");
}

int fbx_tomo_simulate_symmetrized(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const double* truth,
                                  const double* confusion, int symm_type, int64_t n_shots, uint64_t seed, int64_t first_item,
                                  double* expect_out, double* counts_out, double* std_err_out, double* exact_out, double* prob_out,
                                  uint32_t* hist_out, int32_t* status_out) {
    FBX_TRY(toms_check(design, grouping, B, truth, confusion, symm_type, n_shots, first_item, expect_out, counts_out, std_err_out,
                       exact_out, prob_out, hist_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t n = (size_t)B, m = (size_t)design->dev.m, d = (size_t)1 << design->dev.n, cells = (size_t)grouping->dev.G * d;
    HostIO io; SimOut o; double *dt, *dcf, *dp; uint32_t* dh;
    FBX_TRY(io.in(truth, n * (size_t)tomo_truth_len(design->dev), &dt));
    FBX_TRY(io.in(confusion, n * d * d, &dcf));
    FBX_TRY(o.stage(io, n, n * m, expect_out, counts_out, std_err_out, exact_out, status_out));
    FBX_TRY(io.out_opt(prob_out, n * cells * d, &dp));
    FBX_TRY(io.out_opt(hist_out, n * cells, &dh));
    FBX_TRY(fbx_tomo_simulate_symmetrized_dev(design, grouping, B, dt, dcf, symm_type, n_shots, seed, first_item, o.expect, o.counts,
                                              o.std_err, o.exact, dp, dh, o.status));
    return io.finish();
}

int fbx_tomo_simulate_calibration_dev(const fbx_design* design, int64_t B, const double* d_confusion, int symm_type,
                                      int64_t cal_shots, uint64_t seed, int64_t first_item, double* d_cal_mean_out,
                                      double* d_cal_var_out, double* d_cal_exact_out, double* d_cal_counts_out,
                                      int32_t* d_status_out) {
    FBX_TRY(tomc_check(design, B, d_confusion, symm_type, cal_shots, first_item, d_cal_mean_out, d_cal_var_out, d_cal_exact_out,
                       d_cal_counts_out));
    FBX_TRY(ensure_device());
    FBX_TRY(toms_calibrations(design));
    if (B == 0) return FBX_OK;
    const SymmOut out{d_cal_mean_out, d_cal_counts_out, d_cal_var_out, d_cal_exact_out, nullptr, nullptr};
    return toms_launch<true>(design, GroupingDev{}, (const int*)design->cal_slab, (int)design->cal_pauli_host.size(), B, nullptr,
                             d_confusion, symm_type, cal_shots, seed, first_item, out, d_status_out, "fbx_tomo_simulate_calibration");
}

int fbx_tomo_simulate_calibration(const fbx_design* design, int64_t B, const double* confusion, int symm_type, int64_t cal_shots,
                                  uint64_t seed, int64_t first_item, double* cal_mean_out, double* cal_var_out,
                                  double* cal_exact_out, double* cal_counts_out, int32_t* status_out) {
    FBX_TRY(tomc_check(design, B, confusion, symm_type, cal_shots, first_item, cal_mean_out, cal_var_out, cal_exact_out,
                       cal_counts_out));
    FBX_TRY(ensure_device());
    FBX_TRY(toms_calibrations(design));
    if (B == 0) return FBX_OK;
    const size_t n = (size_t)B, d = (size_t)1 << design->dev.n, nc = design->cal_pauli_host.size();
    HostIO io; double *dcf, *dm, *dv, *dx, *dc; int32_t* dst;
    FBX_TRY(io.in(confusion, n * d * d, &dcf));
    FBX_TRY(io.out_opt(cal_mean_out, n * nc, &dm));
    FBX_TRY(io.out_opt(cal_var_out, n * nc, &dv));
    FBX_TRY(io.out_opt(cal_exact_out, n * nc, &dx));
    FBX_TRY(io.out_opt(cal_counts_out, n * nc, &dc));
    FBX_TRY(io.out_opt(status_out, n, &dst));
    FBX_TRY(fbx_tomo_simulate_calibration_dev(design, B, dcf, symm_type, cal_shots, seed, first_item, dm, dv, dx, dc, dst));
    return io.finish();
}

}  // fbx C ABI
