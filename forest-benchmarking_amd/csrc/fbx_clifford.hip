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
// a signed permutation: perm (16 x 4 bits) and a mask of the negative columns.
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
#include "fbx_common.hpp"

namespace fbx {

constexpr uint32_t CL_PHASE_LUT = 0x344CD000u;    // 2-bit exponents of a b = i^ph P_(a ^ b), entry 4 a + b: XY = iZ, YZ = iX, ZX = iY
constexpr int RB_MAX_G = 16;

// exponent of i (unreduced) in the product of the Paulis with indices a, b < 16
__host__ __device__ __forceinline__ uint32_t cl_mul_phase(uint32_t a, uint32_t b) {
    return ((CL_PHASE_LUT >> (2 * ((a & 12u) | (b >> 2)))) & 3u) + ((CL_PHASE_LUT >> (2 * (((a & 3u) << 2) | (b & 3u)))) & 3u);
}

template <int NQ> struct ClGroup;
template <> struct ClGroup<1> { static constexpr uint32_t order = 24, identity = 1u | (3u << 5); };
template <> struct ClGroup<2> { static constexpr uint32_t order = 11520, identity = 4u | (12u << 5) | (1u << 10) | (3u << 15); };

template <int NQ>
__host__ __device__ __forceinline__ uint32_t cl_generator(int j) {       // Pauli index of X_0, Z_0[, X_1, Z_1]
    return (ClGroup<NQ>::identity >> (5 * j)) & 15u;
}

// every unused bit zero; images of X_q and Z_q anticommute; images of different qubits commute
template <int NQ>
__host__ __device__ __forceinline__ bool cl_valid(uint32_t w) {
    bool ok = (w >> (10 * NQ)) == 0u;
    uint32_t p[2 * NQ];
#pragma unroll
    for (int j = 0; j < 2 * NQ; ++j) { p[j] = (w >> (5 * j)) & 15u; if (NQ == 1) ok = ok && p[j] < 4u; }
#pragma unroll
    for (int i = 0; i < 2 * NQ; ++i)
#pragma unroll
        for (int j = i + 1; j < 2 * NQ; ++j)
            ok = ok && ((cl_mul_phase(p[i], p[j]) & 1u) == ((i >> 1) == (j >> 1) ? 1u : 0u));
    return ok;
}

// The signed permutation of a valid word: C P_k C^+ = (neg bit k ? -1 : +1) P_perm[k], perm[k] in bits [4 k, 4 k + 4).
template <int NQ>
__host__ __device__ __forceinline__ void cl_table(uint32_t w, unsigned long long& perm, uint32_t& neg) {
    uint32_t qi[NQ][4], qp[NQ][4];                 // per qubit: image of I, X, Y, Z as (index, exponent of i)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const uint32_t px = (w >> (10 * q)) & 15u, sx = (w >> (10 * q + 4)) & 1u;
        const uint32_t pz = (w >> (10 * q + 5)) & 15u, sz = (w >> (10 * q + 9)) & 1u;
        qi[q][0] = 0u; qp[q][0] = 0u;
        qi[q][1] = px; qp[q][1] = 2u * sx;
        qi[q][3] = pz; qp[q][3] = 2u * sz;
        qi[q][2] = px ^ pz; qp[q][2] = 1u + 2u * (sx + sz) + cl_mul_phase(px, pz);      // Y = i X Z
    }
    perm = 0ull; neg = 0u;
#pragma unroll
    for (int k = 0; k < (1 << (2 * NQ)); ++k) {
        uint32_t idx, ph;
        if constexpr (NQ == 1) { idx = qi[0][k]; ph = qp[0][k]; }
        else {
            const uint32_t a = qi[0][k >> 2], b = qi[1][k & 3];
            idx = a ^ b; ph = qp[0][k >> 2] + qp[1][k & 3] + cl_mul_phase(a, b);
        }
        perm |= (unsigned long long)idx << (4 * k);
        neg |= ((ph >> 1) & 1u) << k;
    }
}

// a after b: the images of b's images under a
template <int NQ>
__host__ __device__ __forceinline__ uint32_t cl_compose(unsigned long long perm_a, uint32_t neg_a, uint32_t b) {
    uint32_t out = 0u;
#pragma unroll
    for (int j = 0; j < 2 * NQ; ++j) {
        const uint32_t p = (b >> (5 * j)) & 15u, s = (b >> (5 * j + 4)) & 1u;
        out |= ((uint32_t)((perm_a >> (4 * p)) & 15ull) | ((s ^ ((neg_a >> p) & 1u)) << 4)) << (5 * j);
    }
    return out;
}

// the inverse from the table: generator g is the image of the one Pauli k with perm[k] = g, with the same sign
template <int NQ>
__host__ __device__ __forceinline__ uint32_t cl_inverse(unsigned long long perm, uint32_t neg) {
    uint32_t out = 0u;
#pragma unroll
    for (int j = 0; j < 2 * NQ; ++j) {
        const uint32_t g = cl_generator<NQ>(j);
#pragma unroll
        for (int k = 1; k < (1 << (2 * NQ)); ++k)
            if ((uint32_t)((perm >> (4 * k)) & 15ull) == g) out |= ((uint32_t)k | (((neg >> k) & 1u) << 4)) << (5 * j);
    }
    return out;
}

// fbx/clifford.py from_index: idx = signs + 4^n r; the images are chosen one after the other, the c-th candidate in ascending Pauli
// index that commutes with the images of the earlier qubits and (for Z_q) anticommutes with the image of X_q.  idx < order.
template <int NQ>
__host__ __device__ __forceinline__ uint32_t cl_from_index(uint32_t idx) {
    const uint32_t signs = idx & ((1u << (2 * NQ)) - 1u);
    uint32_t r = idx >> (2 * NQ), chosen[2 * NQ], out = 0u;
#pragma unroll
    for (int j = 0; j < 2 * NQ; ++j) {
        const uint32_t base = NQ == 1 ? (j == 0 ? 3u : 2u) : (j == 0 ? 15u : j == 1 ? 8u : j == 2 ? 3u : 2u);
        uint32_t c = r % base, pick = 0u;
        r /= base;
        // ascending scan with a running count (no early exit: every lane runs the same 4^n - 1 steps)
        uint32_t seen = 0u;
#pragma unroll
        for (uint32_t cand = 1u; cand < (1u << (2 * NQ)); ++cand) {
            bool ok = true;
#pragma unroll
            for (int e = 0; e < 2 * (j >> 1); ++e) ok = ok && (cl_mul_phase(cand, chosen[e]) & 1u) == 0u;
            if (j & 1) ok = ok && (cl_mul_phase(cand, chosen[j - 1]) & 1u) == 1u;
            if (ok) { if (seen == c) pick = cand; ++seen; }
        }
        chosen[j] = pick;
        out |= (pick | (((signs >> j) & 1u) << 4)) << (5 * j);
    }
    return out;
}

#if defined(__HIPCC__)
// Uniform on range(N), N < 2^16: x N / 2^32 of a 32-bit word x, rejected when the low half of the product falls below 2^32 mod N
// (Lemire, "Fast random integer generation in an interval", 2019) -- every value keeps exactly floor(2^32 / N) words.  Draw
// `draw` of sequence b takes the four words of block (b, draw, attempt) in turn; a rejection has probability < N / 2^32 < 3e-6, so
// eight blocks (32 words) never run out in practice, and the loop is bounded for the sake of a bound.
__device__ __forceinline__ uint32_t cl_draw(unsigned long long seed, long long b, uint32_t draw, uint32_t N) {
    const uint32_t thresh = (0u - N) % N;
    unsigned long long m = 0ull;
    for (uint32_t attempt = 0u; attempt < 8u; ++attempt) {
        uint32_t c[4] = {(uint32_t)b, (uint32_t)((unsigned long long)b >> 32), draw, 0x52420000u + attempt};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            m = (unsigned long long)c[w] * N;
            if ((uint32_t)m >= thresh) return (uint32_t)(m >> 32);
        }
    }
    return (uint32_t)(m >> 32);
}

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
