// fbx_clifford.hip -- the 1- and 2-qubit Clifford groups on the device, randomized-benchmarking sequences and their simulation
// under Pauli-transfer-matrix noise.
//
// The reference hands this to quilc through a BenchmarkConnection (randomized_benchmarking.py:105-174: sample a uniform Clifford,
// compose, invert); here it is integer arithmetic on packed element words (include/fbx.h, "Clifford elements"; the host mirror is
// fbx/clifford.py and the two agree word for word).
//
// Element word: the signed Pauli images of X_0, Z_0[, X_1, Z_1], five bits each (4 bits Pauli index, 1 sign bit).  The Pauli
// index of the project (digits I X Y Z = 0 1 2 3, qubit 0 most significant) is linear over GF(2): X = 01, Z = 11, Y = X ^ Z = 10,
// so the index of a product of Paulis is the XOR of the indices, and only the power of i needs arithmetic -- two bits per pair of
// single-qubit factors, looked up in one 32-bit constant (cl_mul_phase).  cl_table turns a word into its Pauli transfer matrix,
// a signed permutation: perm (16 x 4 bits) and a mask of the negative columns.  These helpers and the draw of a sequence's
// stream are in fbx_clifford_elems.hpp, which fbx_rb_acquire.hip (the fused acquisition) shares.
//
// rb_sequences_kernel: a lane per sequence.  Sequence b draws from the Philox4x32-10 stream (key = seed, counter = (b, draw,
// attempt)), so its content depends on (seed, b) only.  A draw maps a 32-bit word onto range(|group|) by multiply-high with
// rejection (Lemire): exactly uniform.
//
// rb_simulate_kernel (the hot path): a lane per sequence, 256-thread workgroups, the Pauli vector of the lane in registers.  A
// step is (1) the element's signed permutation and (2) the noise PTM.  (1) is a lane-varying scatter, which registers cannot
// do (a register array under a lane-varying index goes to scratch): the lane writes its d^2 values to ITS column of an LDS
// array vec[k][256] at the permuted k and reads them back in order -- the bank of vec[k][tid] depends on tid alone, so lanes
// never conflict whatever their permutations.  (2) reads the PTM of the step's noise id from LDS (all G of them are staged at
// kernel entry): every lane of a wavefront that agrees on the id reads the same address, a broadcast.  Lanes whose sequences
// are shorter idle until the longest of the wavefront is done.  A lane touches no other lane's data: a NaN, a bad element or a
// bad noise id stays in its sequence.
#include "fbx_clifford_elems.hpp"

namespace fbx {

constexpr int RB_MAX_G = 16;

#if defined(__HIPCC__)
template <int NQ>
__global__ void __launch_bounds__(256)
clifford_from_index_kernel(long long B, const uint32_t* __restrict__ idx, uint32_t* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < B; i += (long long)gridDim.x * blockDim.x) {
        const uint32_t v = idx[i];
        out[i] = v < ClGroup<NQ>::order ? cl_from_index<NQ>(v) : FBX_CLIFFORD_NONE;      // only the _dev form can meet the second
    }
}

template <int NQ>
__global__ void __launch_bounds__(256)
rb_sequences_kernel(long long B, const long long* __restrict__ offsets, unsigned long long seed, uint32_t interleaved, int self_inverting,
                    uint32_t* __restrict__ elems, uint8_t* __restrict__ noise_ids) {
    const bool irb = interleaved != FBX_CLIFFORD_NONE;
    for (long long b = blockIdx.x * (long long)blockDim.x + threadIdx.x; b < B; b += (long long)gridDim.x * blockDim.x) {
        const long long o0 = offsets[b], L = offsets[b + 1] - o0;
        uint32_t total = ClGroup<NQ>::identity;                 // everything so far, later elements on the left
        unsigned long long perm; uint32_t neg;
        for (long long i = 0; i < L; ++i) {
            uint32_t e; uint8_t id = 0;
            if (self_inverting && i == L - 1) {
                cl_table<NQ>(total, perm, neg);
                e = cl_inverse<NQ>(perm, neg);
            } else if (irb && (i & 1)) {
                e = interleaved; id = 1;
            } else {
                e = cl_from_index<NQ>(cl_draw(seed, b, (uint32_t)(irb ? i >> 1 : i), ClGroup<NQ>::order));
            }
            elems[o0 + i] = e;
            if (noise_ids) noise_ids[o0 + i] = id;
            cl_table<NQ>(e, perm, neg);
            total = cl_compose<NQ>(perm, neg, total);
        }
    }
}

template <int NQ>
__global__ void __launch_bounds__(256)
rb_simulate_kernel(long long B, const long long* __restrict__ offsets, const uint32_t* __restrict__ elems,
                   const uint8_t* __restrict__ noise_ids, int G, const double* __restrict__ ptms, const double* __restrict__ prep,
                   double* __restrict__ out) {
    constexpr int D = 1 << (2 * NQ);
    extern __shared__ __attribute__((aligned(16))) double rb_smem[];
    double* vec = rb_smem;                     // [D][256]: column tid belongs to lane tid alone
    double* lam = rb_smem + D * 256;           // [G][D][D]
    const int tid = threadIdx.x;
    for (int i = tid; i < G * D * D; i += 256) lam[i] = ptms[i];
    __syncthreads();
    for (long long b = blockIdx.x * 256ll + tid; b < B; b += (long long)gridDim.x * 256ll) {
        double v[D];
#pragma unroll
        for (int k = 0; k < D; ++k) v[k] = prep ? prep[k] : (((k & 0x5) ^ ((k >> 1) & 0x5)) == 0 ? 1.0 : 0.0);     // |0..0>: every digit I or Z
        const long long o0 = offsets[b], L = offsets[b + 1] - o0;
        bool bad = L < 0;
        for (long long i = 0; i < L; ++i) {
            const uint32_t w = elems[o0 + i];
            const uint32_t id = noise_ids ? noise_ids[o0 + i] : 0u;
            if (!cl_valid<NQ>(w) || id >= (uint32_t)G) { bad = true; break; }
            unsigned long long perm; uint32_t neg;
            cl_table<NQ>(w, perm, neg);
#pragma unroll
            for (int k = 0; k < D; ++k)
                vec[(int)((perm >> (4 * k)) & 15ull) * 256 + tid] = (neg >> k) & 1u ? -v[k] : v[k];
            double u[D];
#pragma unroll
            for (int k = 0; k < D; ++k) u[k] = vec[k * 256 + tid];
            const double* M = lam + id * (D * D);
#pragma unroll
            for (int r = 0; r < D; ++r) {
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c < D; ++c) acc = fma(M[r * D + c], u[c], acc);
                v[r] = acc;
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) out[b * D + k] = bad ? __longlong_as_double(0x7ff8000000000000ll) : v[k];
    }
}
#endif

static int cl_check_width(int n, const char* who) {
    if (n < 1) { set_error(std::string(who) + ": n_qubits must be 1 or 2"); return FBX_ERR_BAD_ARG; }
    if (n > 2) {
        set_error(std::string(who) + ": the Clifford group engine covers 1 and 2 qubits (got " + std::to_string(n) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    return FBX_OK;
}

static bool cl_word_valid(int n, uint32_t w) { return n == 1 ? cl_valid<1>(w) : cl_valid<2>(w); }

static unsigned rb_grid(int64_t B) {
    const int64_t want = (B + 255) / 256;
    return (unsigned)(want < 256 * 16 ? want : 256 * 16);
}

static int rb_sequences_check(int n, int64_t B, const void* offsets, uint32_t interleaved, const void* elems) {
    FBX_TRY(cl_check_width(n, "fbx_rb_sequences"));
    FBX_REQUIRE(B >= 0, "fbx_rb_sequences: B must not be negative");
    FBX_REQUIRE(interleaved == FBX_CLIFFORD_NONE || cl_word_valid(n, interleaved),
                "fbx_rb_sequences: interleaved_elem is neither a valid element word nor FBX_CLIFFORD_NONE");
    FBX_REQUIRE(B == 0 || (offsets && elems), "fbx_rb_sequences: NULL offsets / elems_out buffer");
    return FBX_OK;
}

static int rb_simulate_check(int n, int64_t B, const void* offsets, int G, const void* ptms, const void* out) {
    FBX_TRY(cl_check_width(n, "fbx_rb_simulate"));
    FBX_REQUIRE(B >= 0, "fbx_rb_simulate: B must not be negative");
    FBX_REQUIRE(G >= 1 && G <= RB_MAX_G, "fbx_rb_simulate: G must be 1..16 noise PTMs");
    FBX_REQUIRE(ptms != nullptr, "fbx_rb_simulate: NULL noise_ptms");
    FBX_REQUIRE(B == 0 || (offsets && out), "fbx_rb_simulate: NULL offsets / out buffer");
    return FBX_OK;
}

// offsets[0] = 0, non-decreasing: the host forms know their buffers' sizes from it
static int rb_offsets_check(int64_t B, const int64_t* offsets, const char* msg) {
    FBX_REQUIRE(offsets[0] == 0, msg);
    for (int64_t b = 0; b < B; ++b) FBX_REQUIRE(offsets[b + 1] >= offsets[b], msg);
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_clifford_from_index_dev(int n_qubits, int64_t B, const uint32_t* d_idx, uint32_t* d_elems_out) {
    FBX_TRY(cl_check_width(n_qubits, "fbx_clifford_from_index"));
    FBX_REQUIRE(B >= 0, "fbx_clifford_from_index: B must not be negative");
    FBX_REQUIRE(B == 0 || (d_idx && d_elems_out), "fbx_clifford_from_index: NULL idx / elems_out buffer");
    if (B == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    if (n_qubits == 1) hipLaunchKernelGGL(clifford_from_index_kernel<1>, dim3(rb_grid(B)), dim3(256), 0, stream(), (long long)B, d_idx, d_elems_out);
    else hipLaunchKernelGGL(clifford_from_index_kernel<2>, dim3(rb_grid(B)), dim3(256), 0, stream(), (long long)B, d_idx, d_elems_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_clifford_from_index(int n_qubits, int64_t B, const uint32_t* idx, uint32_t* elems_out) {
    FBX_TRY(cl_check_width(n_qubits, "fbx_clifford_from_index"));
    FBX_REQUIRE(B >= 0, "fbx_clifford_from_index: B must not be negative");
    FBX_REQUIRE(B == 0 || (idx && elems_out), "fbx_clifford_from_index: NULL idx / elems_out buffer");
    if (B == 0) return FBX_OK;
    const uint32_t order = n_qubits == 1 ? ClGroup<1>::order : ClGroup<2>::order;
    for (int64_t i = 0; i < B; ++i) FBX_REQUIRE(idx[i] < order, "fbx_clifford_from_index: an index is not below the group's order (24 / 11520)");
    FBX_TRY(ensure_device());
    HostIO io; uint32_t *di, *dout;
    FBX_TRY(io.in(idx, (size_t)B, &di)); FBX_TRY(io.out(elems_out, (size_t)B, &dout));
    FBX_TRY(fbx_clifford_from_index_dev(n_qubits, B, di, dout));
    return io.finish();
}

int fbx_rb_sequences_dev(int n_qubits, int64_t B, const int64_t* d_offsets, uint64_t seed, uint32_t interleaved_elem, int self_inverting,
                         uint32_t* d_elems_out, uint8_t* d_noise_id_out) {
    FBX_TRY(rb_sequences_check(n_qubits, B, d_offsets, interleaved_elem, d_elems_out));
    if (B == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    if (n_qubits == 1) hipLaunchKernelGGL(rb_sequences_kernel<1>, dim3(rb_grid(B)), dim3(256), 0, stream(), (long long)B, (const long long*)d_offsets,
                                          (unsigned long long)seed, interleaved_elem, self_inverting, d_elems_out, d_noise_id_out);
    else hipLaunchKernelGGL(rb_sequences_kernel<2>, dim3(rb_grid(B)), dim3(256), 0, stream(), (long long)B, (const long long*)d_offsets,
                            (unsigned long long)seed, interleaved_elem, self_inverting, d_elems_out, d_noise_id_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_rb_sequences(int n_qubits, int64_t B, const int64_t* offsets, uint64_t seed, uint32_t interleaved_elem, int self_inverting,
                     uint32_t* elems_out, uint8_t* noise_id_out) {
    FBX_TRY(rb_sequences_check(n_qubits, B, offsets, interleaved_elem, elems_out));
    if (B == 0) return FBX_OK;
    FBX_TRY(rb_offsets_check(B, offsets, "fbx_rb_sequences: offsets must start at 0 and never decrease"));
    FBX_TRY(ensure_device());
    const size_t total = (size_t)offsets[B];
    HostIO io; int64_t* doff; uint32_t* de; uint8_t* dn;
    FBX_TRY(io.in(offsets, (size_t)B + 1, &doff));
    FBX_TRY(io.out(elems_out, total, &de)); FBX_TRY(io.out_opt(noise_id_out, total, &dn));
    FBX_TRY(fbx_rb_sequences_dev(n_qubits, B, doff, seed, interleaved_elem, self_inverting, de, dn));
    return io.finish();
}

int fbx_rb_simulate_dev(int n_qubits, int64_t B, const int64_t* d_offsets, const uint32_t* d_elems, const uint8_t* d_noise_ids, int G,
                        const double* d_noise_ptms, const double* d_prep, double* d_out) {
    FBX_TRY(rb_simulate_check(n_qubits, B, d_offsets, G, d_noise_ptms, d_out));
    if (B == 0) return FBX_OK;
    FBX_REQUIRE(d_elems != nullptr, "fbx_rb_simulate: NULL elems");
    FBX_TRY(ensure_device());
    const int D = 1 << (2 * n_qubits);
    const size_t lds = sizeof(double) * ((size_t)D * 256 + (size_t)G * D * D);        // n = 2, G = 16: 64 KB
    if (n_qubits == 1) hipLaunchKernelGGL(rb_simulate_kernel<1>, dim3(rb_grid(B)), dim3(256), lds, stream(), (long long)B, (const long long*)d_offsets,
                                          d_elems, d_noise_ids, G, d_noise_ptms, d_prep, d_out);
    else hipLaunchKernelGGL(rb_simulate_kernel<2>, dim3(rb_grid(B)), dim3(256), lds, stream(), (long long)B, (const long long*)d_offsets,
                            d_elems, d_noise_ids, G, d_noise_ptms, d_prep, d_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_rb_simulate(int n_qubits, int64_t B, const int64_t* offsets, const uint32_t* elems, const uint8_t* noise_ids, int G,
                    const double* noise_ptms, const double* prep, double* out) {
    FBX_TRY(rb_simulate_check(n_qubits, B, offsets, G, noise_ptms, out));
    if (B == 0) return FBX_OK;
    FBX_TRY(rb_offsets_check(B, offsets, "fbx_rb_simulate: offsets must start at 0 and never decrease"));
    const size_t total = (size_t)offsets[B];
    FBX_REQUIRE(total == 0 || elems, "fbx_rb_simulate: NULL elems");
    for (size_t i = 0; i < total; ++i) {
        FBX_REQUIRE(cl_word_valid(n_qubits, elems[i]), "fbx_rb_simulate: an element word is not a valid Clifford element");
        FBX_REQUIRE(!noise_ids || noise_ids[i] < G, "fbx_rb_simulate: a noise id is not below G");
    }
    FBX_TRY(ensure_device());
    const size_t D = (size_t)1 << (2 * n_qubits);
    HostIO io; int64_t* doff; uint32_t* de; uint8_t* dn = nullptr; double *dl, *dp = nullptr, *dout;
    FBX_TRY(io.in(offsets, (size_t)B + 1, &doff)); FBX_TRY(io.in(elems, total, &de));
    if (noise_ids) FBX_TRY(io.in(noise_ids, total, &dn));
    FBX_TRY(io.in(noise_ptms, (size_t)G * D * D, &dl));
    if (prep) FBX_TRY(io.in(prep, D, &dp));
    FBX_TRY(io.out(out, (size_t)B * D, &dout));
    FBX_TRY(fbx_rb_simulate_dev(n_qubits, B, doff, de, dn, G, dl, dp, dout));
    return io.finish();
}

}  // extern "C"
