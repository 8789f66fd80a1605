// fbx_tomo_grouping.hpp -- the grouping object (fbx_grouping_create) and the outcome distribution of a group, shared by the
// grouped simulators: fbx_tomo_sim_grouped.hip (fbx_tomo_simulate_grouped) and fbx_tomo_sim_symm.hip (symmetrized readout
// under a joint confusion matrix).  Both evaluate tomog_distribution, so their ideal distributions agree bit for bit.
#pragma once
#include "fbx_sim_shared.hpp"

namespace fbx {

constexpr int TOMOG_THREADS = 256;
constexpr int TOMOG_WAVES = TOMOG_THREADS / 64;
constexpr int TOMOG_MAX_OUTCOMES = 32;              // 2^5: state designs go to 5 qubits
constexpr uint32_t TOMOG_KEY_TAG = 0x544F4D47u;     // "TOMG": keeps the stream apart from fbx_tomo_simulate under one seed

struct GroupingDev {
    int G;
    const int* gstate;        // [G] input-state index (row of DesignDev::Ct)
    const int* gbasis;        // [G] Pauli index of the basis: full weight, Z where no member acts
    const int* mptr;          // [G+1] member ranges
    const int* mk;            // [m] members sorted by group: the caller's setting index
    const uint32_t* msp;      // [m] ... packed (state index << 16 | pauli index), as DesignDev::sp
    const int* mmask;         // [m] ... parity mask: bit t set where base-4 digit t of the Pauli index is not the identity
    const double* mcoef;      // [m] ... coefficient
};

}  // namespace fbx

struct fbx_grouping {
    fbx::GroupingDev dev;
    const fbx_design* design = nullptr;
    int device = -1, epoch = -1;
    void* slab = nullptr;
    std::vector<int> gunion_host;   // [G] the union of the members' parity masks (host copy: what a call is refused on)
};

namespace fbx {

// Steps 1-3 of the contract for the unit (item, group) of the calling wavefront.  Returns the probability of outcome `lane`
// (lanes >= 2^n: unspecified) and leaves the running sum of the clamped probabilities up to and including outcome `lane` in
// *c_mine and the total in *c_last (wave-uniform).  `pw` is 2^n doubles of the wavefront's LDS.
__device__ __forceinline__ double tomog_distribution(const DesignDev& des, const double* __restrict__ truth,
                                                      const double* __restrict__ flip, int state, int basis, int lane,
                                                      double* pw, double* c_mine, double* c_last) {
    const int n = des.n, d = 1 << n;
    double v = 1.0;                                            // t of the empty subset
    if (lane > 0 && lane < d) {
        int keep = 0;
        for (int t = 0; t < n; ++t) if ((lane >> t) & 1) keep |= 3 << (2 * t);
        v = des.kind == FBX_KIND_PROCESS ? tomo_trace_process(truth, des.Ct + (size_t)state * des.D, des.D, basis & keep)
                                         : tomo_trace_state(reinterpret_cast<const cplx*>(truth), n, basis & keep);
    }
    for (int h = 1; h < d; h <<= 1) {                          // p(o) 2^n = sum_T (-1)^{|o & T|} t_T; lanes < 2^n mix among themselves
        const double w = __shfl_xor(v, h);
        v = (lane & h) ? w - v : v + w;
    }
    v *= 1.0 / (double)d;                                      // a power of two: exact
    if (flip) {
        for (int t = 0; t < n; ++t) {                          // bit t is qubit n - 1 - t; [q][0] = P(read 1 | drawn 0), [q][1] = P(read 0 | drawn 1)
            const int q = n - 1 - t;
            const double f0 = flip[2 * q], f1 = flip[2 * q + 1];
            const double w = __shfl_xor(v, 1 << t);
            v = ((lane >> t) & 1) ? fma(1.0 - f1, v, f0 * w) : fma(1.0 - f0, v, f1 * w);
        }
    }
    FBX_WAVE_SYNC();
    if (lane < d) pw[lane] = v;
    FBX_WAVE_SYNC();
    double c = 0.0, mine = 0.0;
    for (int o = 0; o < d; ++o) {                              // one addition per outcome, in outcome order
        const double p = pw[o];
        c += p < 0.0 ? 0.0 : p;                                // max(p, 0), a NaN kept
        if (o == lane) mine = c;
    }
    *c_mine = mine; *c_last = c;
    return v;
}

__device__ __forceinline__ bool tomog_bad_total(double c) { return !(c > 0.0 && c < __builtin_inf()); }

inline int check_grouping(const fbx_grouping* grp, const fbx_design* design, const char* who) {
    if (!grp) { set_error(std::string(who) + ": NULL grouping"); return FBX_ERR_BAD_ARG; }
    if (grp->design != design) { set_error(std::string(who) + ": the grouping was created for another design"); return FBX_ERR_BAD_ARG; }
    if (grp->device != current_device() || grp->epoch != device_epoch()) {
        set_error(std::string(who) + ": the grouping was created on another device; create it again");
        return FBX_ERR_BAD_ARG;
    }
    return FBX_OK;
}

}  // namespace fbx
