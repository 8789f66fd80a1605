// fbx_sample_common.hpp -- what fbx_sample.hip (widths 1..13) and fbx_sample_wide.hip (widths 14..26) share: the argument checks of
// the entry points and the test of a probability.
#pragma once
#include "fbx_common.hpp"

namespace fbx {

#if defined(__HIPCC__)
__device__ __forceinline__ bool sample_bad_probability(double v) { return !(v >= 0.0 && v <= 1.0); }      // NaN included
#endif

// The checks of fbx_sample_bitstrings[_wide][_dev], in the order the header promises: sizes, then the width (`why`: what the range
// is owed to; FBX_ERR_UNSUPPORTED before any buffer is looked at), then the buffers.
inline int sample_check(const char* who, int lo, int hi, const char* why, int n_qubits, int64_t B, int64_t n_shots, const void* probs,
                        int64_t first_item, const void* bits) {
    const std::string w(who);
    FBX_REQUIRE(B >= 0 && n_shots >= 0 && first_item >= 0, w + ": need B >= 0, n_shots >= 0 and first_item >= 0");
    FBX_REQUIRE(n_shots < ((int64_t)1 << 32), w + ": n_shots must be below 2^32 (the shot is one word of the Philox counter)");
    if (n_qubits < lo || n_qubits > hi) {
        set_error(w + ": n_qubits must be " + std::to_string(lo) + ".." + std::to_string(hi) + " (" + why + "; got " +
                  std::to_string(n_qubits) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    FBX_REQUIRE(B == 0 || n_shots == 0 || (probs && bits), w + ": NULL probs / bits_out");
    FBX_REQUIRE(B <= INT64_MAX / (n_shots ? n_shots : 1) / n_qubits, w + ": B * n_shots * n_qubits overflows");
    return FBX_OK;
}

}  // namespace fbx
