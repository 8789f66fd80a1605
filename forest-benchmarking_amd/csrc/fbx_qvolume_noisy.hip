// fbx_qvolume_noisy.hip -- quantum-volume circuits under gate noise: stochastic Pauli-error trajectories.
//
// fbx_qv_noisy_trajectories: T trajectories of each of B circuits of one width.  A trajectory is the circuit of fbx_qv_heavy_outputs
// with, after every gate and with that gate's probability, one of the 15 non-identity Paulis on the gate's pair.  The simulator is
// the one of fbx_qvolume.hip -- the whole state in LDS, swizzled by qv_slot (the bank analysis in that file's header carries over
// unchanged: the Pauli only changes WHICH of a group's four slots an output goes to, and every lane of a group of lanes applies
// the same XOR), one wavefront per trajectory at widths 2..8 (four per workgroup, no workgroup barrier), one workgroup per
// trajectory at widths 9..13 -- and the Pauli costs no pass over the state: qv_apply_gate_pauli (fbx_qv_gate.hpp) folds it into
// the gate's own write-back.  No radix select: the heavy set comes in as the mask fbx_qv_heavy_outputs made of the ideal circuit.
//
// The stream (include/fbx.h): one Philox4x32-10 block per two gates, counter (g low, g high, t, l / 2), all of it wave-uniform
// (scalar ALU; the one comparison in double goes through the VALU and comes back through a readfirstlane).
//
// Units and sums.  The unit of work is (circuit b, segment s): the trajectories t = s * seg .. min(T, (s + 1) * seg) - 1, run one
// after the other by one team.  A thread owns the outputs tid, tid + nth, ... (at most eight) and keeps their running sums over
// the segment in registers -- a second 2^n table does not fit next to the state at width 13 -- so a segment's partial sum is
// summed in the order of t.  With probs_mean_out the segment length is QVN_SEG, a constant, the partial sums go to the workspace
// WS_QV_NOISY [chunk][nseg][2^n] and qvn_mean_kernel adds the segments of an output in the order of s and divides by T: the
// summation order depends on T alone, and no floating-point atomic is involved.  Without probs_mean_out nothing is summed over
// trajectories and every trajectory is a unit of its own.  hprob_traj_out is summed like heavy_prob_out of fbx_qv_heavy_outputs:
// a thread's outputs in ascending order, the lanes by wave_sum, the wavefronts in order.
#include <algorithm>
#include "fbx_common.hpp"
#include "fbx_qv_gate.hpp"

namespace fbx {

constexpr uint32_t QVN_KEY_TAG = 0x51564745u;           // "QVGE": the key tag of this stream (include/fbx.h)
constexpr int QVN_SEG = 4;                               // trajectories per partial sum; part of the summation order of probs_mean_out

struct QvnScratch {
    double red[16];
    unsigned bad[16];
};

template <bool WAVE>
__device__ __forceinline__ void qvn_sync() {
    if constexpr (WAVE) FBX_WAVE_SYNC(); else __syncthreads();
}

// the scalars of a launch (the pointers are kernel arguments of their own: only a `const __restrict__` kernel argument is read
// through scalar loads, and the 4 x 4 matrix of a gate has to be)
struct QvnArgs {
    int n, L, seg;
    long long units, nseg, T, item0, first_item;
    uint32_t k0, k1;
};

#define QVN_POINTER_PARAMS                                                                                                          \
    const uint8_t* __restrict__ pairs, const double* __restrict__ gates, const double* __restrict__ gate_error,                     \
    const unsigned long long* __restrict__ mask, double* __restrict__ part /* [units / nseg][nseg][2^n] of this launch, or NULL */, \
    double* __restrict__ hprob, int* __restrict__ nerr_out, int* __restrict__ status
#define QVN_POINTER_ARGS pairs, gates, gate_error, mask, part, hprob, nerr_out, status

// One team (a wavefront or the workgroup) runs unit u in S (N slots).  OWN: the outputs a thread owns, 2^n / nth -- 8 at width 13, at
// most 4 below; MEAN: running sums over the unit's trajectories are kept (16 registers at OWN = 8 that the other forms do not pay).
template <bool WAVE, bool MEAN, int OWN>
__device__ void qvn_unit(const QvnArgs& A, QVN_POINTER_PARAMS, long long u, cplx* S, QvnScratch* sc, int tid, int nth) {
    const int n = A.n, L = A.L, N = 1 << n, groups = N >> 2, W = N >= 64 ? N >> 6 : 1, lane = tid & 63;
    const long long b = u / A.nseg, s = u - b * A.nseg, item = A.item0 + b, g = A.first_item + item;
    const long long t_begin = s * A.seg, t_end = t_begin + A.seg < A.T ? t_begin + A.seg : A.T;
    const uint32_t g0 = (uint32_t)((unsigned long long)g & 0xFFFFFFFFull), g1 = (uint32_t)((unsigned long long)g >> 32);
    double acc[MEAN ? OWN : 1];
#pragma unroll
    for (int k = 0; k < (MEAN ? OWN : 1); ++k) acc[k] = 0.0;
    unsigned bad_unit = 0;
    for (long long t = t_begin; t < t_end; ++t) {
        for (int i = tid; i < N; i += nth) S[i] = cplx{i == 0 ? 1.0 : 0.0, 0.0};      // slot 0 = element 0
        qvn_sync<WAVE>();
        unsigned bad = 0;
        int nerr = 0;
        uint32_t c[4] = {0u, 0u, 0u, 0u};
        for (int l = 0; l < L; ++l) {
            if ((l & 1) == 0) {
                c[0] = g0; c[1] = g1; c[2] = (uint32_t)t; c[3] = (uint32_t)(l >> 1);
                philox4x32_10(c, A.k0, A.k1);
            }
            const uint32_t xe = (l & 1) ? c[2] : c[0], xp = (l & 1) ? c[3] : c[1];
            const double ge = gate_error[(size_t)item * L + l];
            if (!(ge >= 0.0 && ge <= 1.0)) bad = 1;                                   // NaN included
            int x = 0, z = 0;
            if (uniform((int)((double)xe * 0x1p-32 < ge))) {                            // the rule of the sampler's readout flips
                const int k = 1 + (int)(((unsigned long long)xp * 15ull) >> 32);       // 1..15 = 4 a + c; I X Y Z = 0 1 2 3
                const int a = k >> 2, cc = k & 3;
                x = ((((a + 1) >> 1) & 1) << 1) | (((cc + 1) >> 1) & 1);                // X and Y flip the bit
                z = ((a >> 1) << 1) | (cc >> 1);                                        // Y and Z sign it
                ++nerr;
            }
            const uint8_t* pr = pairs + ((size_t)item * L + l) * 2;
            const int q0 = uniform((int)pr[0]), q1 = uniform((int)pr[1]);
            if (q0 >= n || q1 >= n || q0 == q1) { bad = 1; continue; }                  // wave-uniform; never index outside the state
            qv_apply_gate_pauli(S, groups, n - 1 - q0, n - 1 - q1, gates + ((size_t)item * L + l) * 32, x, z, tid, nth);
            qvn_sync<WAVE>();
        }
        // probabilities in output order: the running sums, the weight on the heavy set, the non-finite check
        double hp = 0.0;
        unsigned lbad = bad;
#pragma unroll
        for (int k = 0; k < OWN; ++k) {
            const int i = tid + k * nth;
            if (i < N) {
                const cplx a = S[qv_slot(i)];
                const double p = a.re * a.re + a.im * a.im;
                if (((unsigned long long)__double_as_longlong(p) & 0x7FF0000000000000ull) == 0x7FF0000000000000ull) lbad = 1;
                if constexpr (MEAN) acc[k] += p;
                if (mask) {
                    const unsigned long long word = mask[(size_t)item * W + (uniform(i >> 6) & (W - 1))];   // one word per wavefront: a scalar load, kept inside the row
                    if ((word >> (i & 63)) & 1ull) hp += p;
                }
            }
        }
        hp = wave_sum(hp);
        unsigned tbad = __ballot(lbad != 0) != 0ull ? 1u : 0u;
        if constexpr (!WAVE) {
            if (lane == 0) { sc->red[tid >> 6] = hp; sc->bad[tid >> 6] = tbad; }
            __syncthreads();
            double sum = 0.0;
            unsigned any = 0;
            for (int w = 0; w < nth >> 6; ++w) { sum += sc->red[w]; any |= sc->bad[w]; }
            hp = sum; tbad = any;                  // (the next write of red / bad comes after the next trajectory's barriers)
        }
        if (tid == 0) {
            if (hprob) hprob[(size_t)item * A.T + t] = tbad ? __builtin_nan("") : hp;
            if (nerr_out) nerr_out[(size_t)item * A.T + t] = tbad ? 0 : nerr;
        }
        bad_unit |= tbad;
        qvn_sync<WAVE>();                           // every read of the state is done before the next trajectory resets it
    }
    if constexpr (MEAN) {
        double* dst = part + (size_t)u * N;
#pragma unroll
        for (int k = 0; k < OWN; ++k) {
            const int i = tid + k * nth;
            if (i < N) dst[i] = bad_unit ? __builtin_nan("") : acc[k];
        }
    }
    if (status && s == 0 && tid == 0) status[item] = (int)bad_unit;
}

extern __shared__ __attribute__((aligned(16))) unsigned char qvn_lds[];

// widths 9..13: one workgroup per trajectory
template <bool MEAN, int OWN>
__global__ void __launch_bounds__(1024) qvn_block_kernel(QvnArgs A, QVN_POINTER_PARAMS) {
    cplx* S = reinterpret_cast<cplx*>(qvn_lds);
    QvnScratch* sc = reinterpret_cast<QvnScratch*>(qvn_lds + (sizeof(cplx) << A.n));
    for (long long u = blockIdx.x; u < A.units; u += gridDim.x)
        qvn_unit<false, MEAN, OWN>(A, QVN_POINTER_ARGS, u, S, sc, (int)threadIdx.x, (int)blockDim.x);
}

// widths 2..8: one wavefront per trajectory, four per workgroup
template <bool MEAN>
__global__ void __launch_bounds__(256) qvn_wave_kernel(QvnArgs A, QVN_POINTER_PARAMS) {
    const int wave = uniform((int)(threadIdx.x >> 6));
    cplx* S = reinterpret_cast<cplx*>(qvn_lds + (sizeof(cplx) << A.n) * wave);
    for (long long u = (long long)blockIdx.x * 4 + wave; u < A.units; u += (long long)gridDim.x * 4)
        qvn_unit<true, MEAN, 4>(A, QVN_POINTER_ARGS, u, S, nullptr, (int)(threadIdx.x & 63), 64);
}

// probs_mean_out of `count` = items x 2^n outputs: the segments of an output in order, then one division by T
__global__ void __launch_bounds__(256) qvn_mean_kernel(int n, long long count, long long nseg, long long T, const double* __restrict__ part,
                                                       double* __restrict__ out) {
    const long long N = 1ll << n;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < count; idx += (long long)gridDim.x * 256) {
        const long long b = idx >> n, i = idx & (N - 1);
        const double* p = part + (size_t)(b * nseg) * N + i;
        double sum = 0.0;
        for (long long s = 0; s < nseg; ++s) sum += p[(size_t)s * N];
        out[idx] = sum / (double)T;
    }
}

static int qvn_check(int n_qubits, int64_t B, int L, int64_t T, const void* pairs, const void* gates, const void* gate_error,
                     const void* heavy_mask, int64_t first_item, const void* probs_mean, const void* hprob_traj, const void* n_errors) {
    FBX_REQUIRE(B >= 0 && L >= 0 && T >= 0 && first_item >= 0, "fbx_qv_noisy_trajectories: need B >= 0, L >= 0, T >= 0 and first_item >= 0");
    FBX_REQUIRE(T < ((int64_t)1 << 32), "fbx_qv_noisy_trajectories: T must be below 2^32 (the trajectory is one counter word of the stream)");
    FBX_REQUIRE(B == 0 || T == 0 || L == 0 || (pairs && gates && gate_error), "fbx_qv_noisy_trajectories: NULL pairs / gates / gate_error");
    FBX_REQUIRE(probs_mean || hprob_traj || n_errors, "fbx_qv_noisy_trajectories: no result asked for");
    FBX_REQUIRE(!hprob_traj || heavy_mask, "fbx_qv_noisy_trajectories: hprob_traj_out needs heavy_mask");
    if (n_qubits < 2 || n_qubits > 13) {
        set_error("fbx_qv_noisy_trajectories: n_qubits must be 2..13 (a wider state does not fit the LDS of one CU; got " +
                  std::to_string(n_qubits) + "); a wider trajectory is an ordinary circuit of fbx_qv_heavy_outputs_wide once its "
                  "Paulis are folded into its gates");
        return FBX_ERR_UNSUPPORTED;
    }
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_qv_noisy_trajectories_dev(int n_qubits, int64_t B, int L, int64_t T, const uint8_t* d_pairs, const double* d_gates,
                                  const double* d_gate_error, const uint64_t* d_heavy_mask, uint64_t seed, int64_t first_item,
                                  double* d_probs_mean_out, double* d_hprob_traj_out, int32_t* d_n_errors_out, int32_t* d_status_out) {
    FBX_TRY(qvn_check(n_qubits, B, L, T, d_pairs, d_gates, d_gate_error, d_heavy_mask, first_item, d_probs_mean_out, d_hprob_traj_out,
                      d_n_errors_out));
    FBX_TRY(ensure_device());
    if (B == 0 || T == 0) return FBX_OK;
    const size_t N = (size_t)1 << n_qubits, state = sizeof(cplx) << n_qubits;
    QvnArgs A;
    A.n = n_qubits; A.L = L; A.T = T; A.first_item = first_item;
    A.seg = d_probs_mean_out ? QVN_SEG : 1;
    A.nseg = (T + A.seg - 1) / A.seg;
    A.k0 = (uint32_t)(seed & 0xFFFFFFFFull) ^ QVN_KEY_TAG; A.k1 = (uint32_t)(seed >> 32);
    const unsigned long long* d_mask = (const unsigned long long*)d_heavy_mask;
    double* part = nullptr;
    // the chunk: as many circuits as the workspace cap admits partial sums for, at least one (all of them without probs_mean_out)
    int64_t chunk = B;
    if (d_probs_mean_out) {
        const double per = 8.0 * (double)N * (double)A.nseg;
        chunk = (int64_t)(option_qv_noisy_workspace_mib() * 1048576.0 / per);
        chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, B));
        void* ws = nullptr;
        FBX_TRY(workspace(WS_QV_NOISY, 8 * N * (size_t)A.nseg * (size_t)chunk, &ws));
        part = static_cast<double*>(ws);
    }
    for (int64_t item0 = 0; item0 < B; item0 += chunk) {
        const int64_t cb = std::min<int64_t>(chunk, B - item0);
        A.item0 = item0; A.units = cb * A.nseg;
        if (n_qubits <= 8) {
            const int64_t wgs = (A.units + 3) / 4;
            const unsigned grid = (unsigned)(wgs < 256 * 16 ? wgs : 256 * 16);
            hipLaunchKernelGGL(part ? qvn_wave_kernel<true> : qvn_wave_kernel<false>, dim3(grid), dim3(256), 4 * state, stream(), A, d_pairs,
                               d_gates, d_gate_error, d_mask, part, d_hprob_traj_out, d_n_errors_out, d_status_out);
        } else {
            const size_t lds = state + sizeof(QvnScratch);               // width 13: 128 KiB + 192 B of the 160 KiB
            const int groups = 1 << (n_qubits - 2);
            const unsigned threads = (unsigned)(groups < 1024 ? groups : 1024);
            const unsigned grid = (unsigned)(A.units < 256 * 16 ? A.units : 256 * 16);
            auto kernel = n_qubits == 13 ? (part ? qvn_block_kernel<true, 8> : qvn_block_kernel<false, 8>)
                                         : (part ? qvn_block_kernel<true, 4> : qvn_block_kernel<false, 4>);
            if (lds > 64 * 1024)                                         // widths 12 and 13; below, the default limit holds
                FBX_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, stream(), A, d_pairs, d_gates, d_gate_error, d_mask, part,
                               d_hprob_traj_out, d_n_errors_out, d_status_out);
        }
        FBX_HIP(hipGetLastError());
        if (d_probs_mean_out) {
            const long long count = (long long)cb << n_qubits, blocks = (count + 255) / 256;
            hipLaunchKernelGGL(qvn_mean_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream(), n_qubits, count,
                               A.nseg, (long long)T, (const double*)part, d_probs_mean_out + (size_t)item0 * N);
            FBX_HIP(hipGetLastError());
        }
    }
    return FBX_OK;
}

int fbx_qv_noisy_trajectories(int n_qubits, int64_t B, int L, int64_t T, const uint8_t* pairs, const double* gates,
                              const double* gate_error, const uint64_t* heavy_mask, uint64_t seed, int64_t first_item,
                              double* probs_mean_out, double* hprob_traj_out, int32_t* n_errors_out, int32_t* status_out) {
    FBX_TRY(qvn_check(n_qubits, B, L, T, pairs, gates, gate_error, heavy_mask, first_item, probs_mean_out, hprob_traj_out, n_errors_out));
    FBX_TRY(ensure_device());
    if (B == 0 || T == 0) return FBX_OK;
    const size_t n = (size_t)B, N = (size_t)1 << n_qubits, W = N >= 64 ? N / 64 : 1, n_gates = n * (size_t)L;
    HostIO io; uint8_t* dp; double *dg, *de, *dmean, *dhp; uint64_t* dmask = nullptr; int32_t *dne, *dst;
    FBX_TRY(io.in(pairs, 2 * n_gates, &dp)); FBX_TRY(io.in(gates, 32 * n_gates, &dg)); FBX_TRY(io.in(gate_error, n_gates, &de));
    if (heavy_mask) FBX_TRY(io.in(heavy_mask, n * W, &dmask));
    FBX_TRY(io.out_opt(probs_mean_out, n * N, &dmean)); FBX_TRY(io.out_opt(hprob_traj_out, n * (size_t)T, &dhp));
    FBX_TRY(io.out_opt(n_errors_out, n * (size_t)T, &dne)); FBX_TRY(io.out_opt(status_out, n, &dst));
    FBX_TRY(fbx_qv_noisy_trajectories_dev(n_qubits, B, L, T, dp, dg, de, dmask, seed, first_item, dmean, dhp, dne, dst));
    return io.finish();
}

}  // namespace fbx C ABI
