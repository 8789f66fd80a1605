// fbx_qvolume.hip -- quantum-volume heavy outputs (quantum_volume.py:94-123) and heavy-hitter counts (:322-341), batched.
//
// fbx_qv_heavy_outputs: a state-vector simulator with the whole state in LDS.  A width-n state is 2^n complex128 = 16 B x 2^n
// (n = 13: 128 KiB of the 160 KiB of a CU).  Widths 9..13: one workgroup per circuit (min(1024, 2^n / 4) threads); widths 2..8: one
// WAVEFRONT per circuit, four circuits per workgroup and no workgroup barrier (the LDS operations of one wavefront execute in
// order).  Per gate a thread owns the 4-amplitude groups whose index is its counter with zero bits inserted at the two target
// positions; the amplitudes move as 16-byte LDS accesses and the 4 x 4 matrix is read through wave-uniform (scalar) loads.
//
// LDS banks: a 16-byte read is served in groups of 16 lanes over 64 banks, a 16-byte write in groups of 8 lanes over 32 banks, so
// a group is conflict-free when its element indices differ modulo 16 (8).  A target on one of the least significant index bits
// pins that bit for the whole lane group: stored plainly, one such target makes every access 2-way and two make it 4-way -- and
// at width 13 more than half of all random pairs have one.  The state is therefore stored swizzled (qv_slot): index bit 3 is
// XORed onto slot bits 0..2, bit 4 onto bit 3, bit 5 onto bit 0 and bit 6 onto bit 1.  Over GF(2) the images of index bits 0..4 in
// the four bank-selecting slot bits are then e1, e2, e3, e1+e2+e3+e4, e4 -- any four of them independent, and any three of the first
// four independent modulo e4 -- so EVERY gate with at most one target among the low bits is conflict-free, reads and writes (no
// linear map does that for two low targets as well: it would be a binary MDS code); bits 5 and 6 were chosen by enumeration to
// leave the fewest conflicts among the pairs with two.  scripts/qv_lds_conflicts.py enumerates every (width, pair) with and
// without the swizzle.  The map is linear and a bijection of every aligned block of 128 slots (the identity below 8), so the four
// slots of a group are slot(base) ^ slot(target masks), and passes that do not care about the order run over the slots directly.
//
// Median without a sort: after the last gate the real part of every slot is overwritten with |amp|^2; non-negative doubles
// order like their bit patterns, so the two middle order statistics come from a most-significant-digit radix select (8-bit
// digits, a 256-bin LDS histogram per pass, starting at the first bit in which the smallest and the largest pattern differ)
// for rank N/2 - 1, and one more pass (how many values are <= it, and the smallest one above it) for rank N/2.  Exact.
//
// fbx_qv_count_heavy: a byte-stream reduction in the style of fbx_shots.hip (16-byte loads, runs of 16 shots per lane).
#include "fbx_common.hpp"
#include "fbx_qv_gate.hpp"

namespace fbx {

struct QvScratch {
    unsigned hist[256];
    unsigned long long mn, mx, above;
    unsigned digit, knew, cnt_le, bad, hcount, pad_;
    double red[16];
};

template <bool WAVE>
__device__ __forceinline__ void qv_sync() {
    if constexpr (WAVE) FBX_WAVE_SYNC(); else __syncthreads();
}

// the k-th smallest (k from 0) of the N bit patterns in S[.].re, all of them between mn and mx
template <bool WAVE>
__device__ unsigned long long qv_select(const cplx* S, int N, unsigned k, unsigned long long mn, unsigned long long mx,
                                        QvScratch* sc, int tid, int nth) {
    const unsigned long long diff = mn ^ mx;
    if (diff == 0) return mn;
    int hi = 63 - __clzll((long long)diff);                            // the highest bit in which two values differ
    unsigned long long pmask = ~((2ull << hi) - 1ull);                // (hi = 63: no common bits)
    unsigned long long prefix = mn & pmask;
    while (hi >= 0) {
        const int shift = hi >= 7 ? hi - 7 : 0;
        const unsigned dmask = (1u << (hi - shift + 1)) - 1u;
        for (int i = tid; i < 256; i += nth) sc->hist[i] = 0;
        qv_sync<WAVE>();
        for (int i = tid; i < N; i += nth) {
            const unsigned long long x = (unsigned long long)__double_as_longlong(S[i].re);
            if ((x & pmask) == prefix) atomicAdd(&sc->hist[(unsigned)(x >> shift) & dmask], 1u);
        }
        qv_sync<WAVE>();
        if (tid < 64) {                                                 // the first wavefront: four bins per lane
            const unsigned c0 = sc->hist[4 * tid], c1 = sc->hist[4 * tid + 1], c2 = sc->hist[4 * tid + 2], c3 = sc->hist[4 * tid + 3];
            const unsigned s = c0 + c1 + c2 + c3;
            const unsigned incl = wave_scan_u32(s, tid), excl = incl - s;
            if (excl <= k && k < incl) {                                // exactly one lane
                unsigned r = k - excl, d = 4 * tid;
                if (r >= c0) { r -= c0; ++d; if (r >= c1) { r -= c1; ++d; if (r >= c2) { r -= c2; ++d; } } }
                sc->digit = d; sc->knew = r;
            }
        }
        qv_sync<WAVE>();
        prefix |= (unsigned long long)sc->digit << shift;
        pmask |= (unsigned long long)dmask << shift;
        k = sc->knew;                          // (the next write of digit / knew comes two barriers later)
        hi = shift - 1;
    }
    return prefix;
}

// One team (a wavefront or the workgroup) simulates circuit `item` in S (N slots) and writes what was asked for.
template <bool WAVE>
__device__ void qv_circuit(int n, long long item, int L, const uint8_t* __restrict__ pairs, const double* __restrict__ gates,
                           double* __restrict__ probs_out, double* __restrict__ median_out,
                           unsigned long long* __restrict__ mask_out, double* __restrict__ hprob_out, int* __restrict__ hcount_out,
                           cplx* S, QvScratch* sc, int tid, int nth) {
    const int N = 1 << n, groups = N >> 2;
    for (int i = tid; i < N; i += nth) S[i] = cplx{i == 0 ? 1.0 : 0.0, 0.0};          // slot 0 = element 0
    if (tid == 0) { sc->mn = ~0ull; sc->mx = 0ull; sc->above = ~0ull; sc->cnt_le = 0; sc->bad = 0; sc->hcount = 0; }
    qv_sync<WAVE>();
    unsigned bad_pair = 0;
    for (int l = 0; l < L; ++l) {
        const uint8_t* pr = pairs + ((size_t)item * L + l) * 2;
        const int q0 = uniform((int)pr[0]), q1 = uniform((int)pr[1]);
        if (q0 >= n || q1 >= n || q0 == q1) { bad_pair = 1; continue; }               // wave-uniform; never index outside the state
        const int p0 = n - 1 - q0, p1 = n - 1 - q1;                                   // qubit 0 = most significant bit
        qv_apply_gate(S, groups, p0, p1, gates + ((size_t)item * L + l) * 32, tid, nth);               // fbx_qv_gate.hpp
        qv_sync<WAVE>();
    }
    // amplitudes -> probabilities (in the real part of the slot), smallest / largest pattern, non-finite check
    unsigned long long lmn = ~0ull, lmx = 0ull;
    unsigned lbad = bad_pair;
    for (int i = tid; i < N; i += nth) {
        const cplx a = S[i];
        const double p = a.re * a.re + a.im * a.im;
        S[i].re = p;
        const unsigned long long x = (unsigned long long)__double_as_longlong(p);
        if ((x & 0x7FF0000000000000ull) == 0x7FF0000000000000ull) lbad = 1;
        lmn = x < lmn ? x : lmn; lmx = x > lmx ? x : lmx;
    }
    atomicMin(&sc->mn, lmn); atomicMax(&sc->mx, lmx);
    if (lbad) atomicOr(&sc->bad, 1u);
    qv_sync<WAVE>();
    const bool bad = sc->bad != 0;
    if (probs_out)
        for (int i = tid; i < N; i += nth) probs_out[(size_t)item * N + i] = bad ? __builtin_nan("") : S[qv_slot(i)].re;
    const int W = N >= 64 ? N >> 6 : 1;
    if (bad) {                                       // a poisoned item: NaN results, an empty heavy set; nothing else is touched
        if (tid == 0) {
            if (median_out) median_out[item] = __builtin_nan("");
            if (hprob_out) hprob_out[item] = __builtin_nan("");
            if (hcount_out) hcount_out[item] = 0;
        }
        if (mask_out)
            for (int w = tid; w < W; w += nth) mask_out[(size_t)item * W + w] = 0ull;
        qv_sync<WAVE>();
        return;
    }
    const unsigned k1 = (unsigned)(N / 2 - 1), k2 = (unsigned)(N / 2);
    const unsigned long long mn = sc->mn, mx = sc->mx;
    const unsigned long long v1 = qv_select<WAVE>(S, N, k1, mn, mx, sc, tid, nth);
    {
        unsigned c = 0;
        unsigned long long ab = ~0ull;
        for (int i = tid; i < N; i += nth) {
            const unsigned long long x = (unsigned long long)__double_as_longlong(S[i].re);
            if (x <= v1) ++c; else ab = x < ab ? x : ab;
        }
        if (c) atomicAdd(&sc->cnt_le, c);
        if (ab != ~0ull) atomicMin(&sc->above, ab);
    }
    qv_sync<WAVE>();
    const unsigned long long v2 = sc->cnt_le > k2 ? v1 : sc->above;
    const double median = 0.5 * (__longlong_as_double((long long)v1) + __longlong_as_double((long long)v2));
    // heavy outputs: strictly above the median; mask word w holds outputs 64 w .. 64 w + 63
    double hp = 0.0;
    unsigned hc = 0;
    const int lane = tid & 63;
    for (int i0 = tid & ~63; i0 < N; i0 += nth) {
        const int i = i0 + lane;
        const double p = i < N ? S[qv_slot(i)].re : 0.0;
        const bool heavy = i < N && p > median;
        const unsigned long long word = __ballot(heavy);
        if (heavy) { hp += p; ++hc; }
        if (mask_out && lane == 0) mask_out[(size_t)item * W + (i0 >> 6)] = word;
    }
    if (hprob_out) {                                // one fixed summation order: lanes (wave_sum), then wavefronts in order
        hp = wave_sum(hp);
        if constexpr (!WAVE) {
            if (lane == 0) sc->red[tid >> 6] = hp;
            __syncthreads();
            double s = 0.0;
            for (int w = 0; w < nth >> 6; ++w) s += sc->red[w];
            hp = s;
        }
    }
    if (hcount_out) {
        if (hc) atomicAdd(&sc->hcount, hc);
        qv_sync<WAVE>();
    }
    if (tid == 0) {
        if (median_out) median_out[item] = median;
        if (hprob_out) hprob_out[item] = hp;
        if (hcount_out) hcount_out[item] = (int)sc->hcount;
    }
    qv_sync<WAVE>();                                // the scratch and the state are reused by the team's next circuit
}

extern __shared__ __attribute__((aligned(16))) unsigned char qv_lds[];

// widths 9..13: one workgroup per circuit
__global__ void __launch_bounds__(1024)
qv_block_kernel(int n, long long B, int L, const uint8_t* __restrict__ pairs, const double* __restrict__ gates,
                double* __restrict__ probs_out, double* __restrict__ median_out, unsigned long long* __restrict__ mask_out,
                double* __restrict__ hprob_out, int* __restrict__ hcount_out) {
    cplx* S = reinterpret_cast<cplx*>(qv_lds);
    QvScratch* sc = reinterpret_cast<QvScratch*>(qv_lds + (sizeof(cplx) << n));
    for (long long item = blockIdx.x; item < B; item += gridDim.x)
        qv_circuit<false>(n, item, L, pairs, gates, probs_out, median_out, mask_out, hprob_out, hcount_out, S, sc,
                          (int)threadIdx.x, (int)blockDim.x);
}

// widths 2..8: one wavefront per circuit, four per workgroup
__global__ void __launch_bounds__(256)
qv_wave_kernel(int n, long long B, int L, const uint8_t* __restrict__ pairs, const double* __restrict__ gates,
               double* __restrict__ probs_out, double* __restrict__ median_out, unsigned long long* __restrict__ mask_out,
               double* __restrict__ hprob_out, int* __restrict__ hcount_out) {
    const int wave = uniform((int)(threadIdx.x >> 6));
    const size_t per_team = (sizeof(cplx) << n) + sizeof(QvScratch);
    cplx* S = reinterpret_cast<cplx*>(qv_lds + per_team * wave);
    QvScratch* sc = reinterpret_cast<QvScratch*>(qv_lds + per_team * wave + (sizeof(cplx) << n));
    for (long long item = (long long)blockIdx.x * 4 + wave; item < B; item += (long long)gridDim.x * 4)
        qv_circuit<true>(n, item, L, pairs, gates, probs_out, median_out, mask_out, hprob_out, hcount_out, S, sc,
                         (int)(threadIdx.x & 63), 64);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// heavy-hitter counts: shot row -> integer (first column most significant, utils.py:32-42) -> one bit of the circuit's mask.
// Only bit 0 of every byte is read.
__device__ __forceinline__ int qv_is_heavy(const unsigned long long* __restrict__ mask, unsigned idx) {
    return (int)((mask[idx >> 6] >> (idx & 63)) & 1ull);
}

template <int NQ>
__device__ long long qv_count_record(const uint8_t* __restrict__ bits, long long n_shots, const unsigned long long* __restrict__ mask,
                                     int tid, int nth) {
    long long cnt = 0;
    // runs of 16 shots = NQ 16-byte vectors per lane, from the first shot that starts on a 16-byte boundary (a record at a
    // multiple of NQ bytes from an aligned base always has one among its first 16); the shots around the runs go byte-wise
    long long head = n_shots, runs = 0;
    for (int s = 0; s < 16; ++s)
        if ((((uintptr_t)bits + (uintptr_t)(s * NQ)) & 15) == 0) { head = s; break; }
    if (head < n_shots) {
        runs = (n_shots - head) / 16;
        const ulonglong2* v = reinterpret_cast<const ulonglong2*>(bits + head * NQ);
        for (long long r = tid; r < runs; r += nth) {
            unsigned long long x[2 * NQ];
#pragma unroll
            for (int w = 0; w < NQ; ++w) { const ulonglong2 t = v[r * NQ + w]; x[2 * w] = t.x; x[2 * w + 1] = t.y; }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                unsigned idx = 0;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int byte = j * NQ + q;
                    idx |= (unsigned)((x[byte >> 3] >> (8 * (byte & 7))) & 1ull) << (NQ - 1 - q);
                }
                cnt += qv_is_heavy(mask, idx);
            }
        }
    } else head = n_shots;
    const long long tail0 = head + runs * 16, rest = head + (n_shots - tail0);
    for (long long k = tid; k < rest; k += nth) {
        const long long s = k < head ? k : tail0 + (k - head);
        unsigned idx = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) idx |= (unsigned)(bits[s * NQ + q] & 1) << (NQ - 1 - q);
        cnt += qv_is_heavy(mask, idx);
    }
    return cnt;
}

template <int NQ, bool PER_WAVE>
__global__ void __launch_bounds__(256)
qv_count_kernel(long long B, long long n_shots, const uint8_t* __restrict__ bits, const unsigned long long* __restrict__ mask,
                long long* __restrict__ counts_out) {
    __shared__ long long part[4];
    constexpr int W = NQ >= 6 ? (1 << NQ) / 64 : 1;
    const int tid = PER_WAVE ? (threadIdx.x & 63) : threadIdx.x, nth = PER_WAVE ? 64 : 256;
    const long long first = PER_WAVE ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
    const long long stride = PER_WAVE ? (long long)gridDim.x * 4 : gridDim.x;
    for (long long b = first; b < B; b += stride) {
        const long long cnt = qv_count_record<NQ>(bits + b * n_shots * NQ, n_shots, mask + b * W, tid, nth);
        long long total = (long long)wave_sum((double)cnt);              // exact: counts stay below 2^53
        if (!PER_WAVE) {
            __syncthreads();
            if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = total;
            __syncthreads();
            total = part[0] + part[1] + part[2] + part[3];
        }
        if (tid == 0) counts_out[b] = total;
    }
}

template <int NQ>
static int launch_qv_count(int64_t B, int64_t n_shots, const uint8_t* bits, const uint64_t* mask, int64_t* counts) {
    const bool per_wave = n_shots * NQ < FBX_RECORD_WAVE_BYTES && B >= 4;               // short records: a wavefront per circuit (as fbx_shots.hip)
    const int64_t units = per_wave ? (B + 3) / 4 : B;
    const unsigned grid = (unsigned)(units < 256 * 16 ? units : 256 * 16);
    if (per_wave)
        hipLaunchKernelGGL((qv_count_kernel<NQ, true>), dim3(grid), dim3(256), 0, stream(), (long long)B, (long long)n_shots, bits,
                           (const unsigned long long*)mask, (long long*)counts);
    else
        hipLaunchKernelGGL((qv_count_kernel<NQ, false>), dim3(grid), dim3(256), 0, stream(), (long long)B, (long long)n_shots, bits,
                           (const unsigned long long*)mask, (long long*)counts);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

static int qv_check_width(int n_qubits, const char* who) {
    if (n_qubits < 2 || n_qubits > 13) {
        set_error(std::string(who) + ": n_qubits must be 2..13 (a wider state does not fit the LDS of one CU; got " +
                  std::to_string(n_qubits) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    return FBX_OK;
}

static int qv_heavy_outputs_check(int n_qubits, int64_t B, int L, const void* pairs, const void* gates, const void* probs,
                                  const void* median, const void* mask, const void* heavy_prob, const void* heavy_count) {
    FBX_REQUIRE(B >= 0 && L >= 0, "fbx_qv_heavy_outputs: need B >= 0 and L >= 0");
    FBX_REQUIRE(B == 0 || L == 0 || (pairs && gates), "fbx_qv_heavy_outputs: NULL pairs / gates");
    FBX_REQUIRE(probs || median || mask || heavy_prob || heavy_count, "fbx_qv_heavy_outputs: no output asked for");
    return qv_check_width(n_qubits, "fbx_qv_heavy_outputs");
}

static int qv_count_heavy_check(int n_qubits, int64_t B, int64_t n_shots, const void* bits, const void* mask, const void* counts) {
    FBX_REQUIRE(B >= 0 && n_shots >= 0, "fbx_qv_count_heavy: need B >= 0 and n_shots >= 0");
    FBX_REQUIRE(B == 0 || (mask && counts && (bits || n_shots == 0)), "fbx_qv_count_heavy: NULL buffer");
    return qv_check_width(n_qubits, "fbx_qv_count_heavy");
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_qv_heavy_outputs_dev(int n_qubits, int64_t B, int L, const uint8_t* d_pairs, const double* d_gates, double* d_probs_out,
                             double* d_median_out, uint64_t* d_heavy_mask_out, double* d_heavy_prob_out, int32_t* d_heavy_count_out) {
    FBX_TRY(qv_heavy_outputs_check(n_qubits, B, L, d_pairs, d_gates, d_probs_out, d_median_out, d_heavy_mask_out, d_heavy_prob_out,
                                   d_heavy_count_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t state = sizeof(cplx) << n_qubits;
    if (n_qubits <= 8) {
        const size_t lds = 4 * (state + sizeof(QvScratch));
        const int64_t units = (B + 3) / 4;
        const unsigned grid = (unsigned)(units < 256 * 16 ? units : 256 * 16);
        hipLaunchKernelGGL(qv_wave_kernel, dim3(grid), dim3(256), lds, stream(), n_qubits, (long long)B, L, d_pairs, d_gates,
                           d_probs_out, d_median_out, (unsigned long long*)d_heavy_mask_out, d_heavy_prob_out, d_heavy_count_out);
    } else {
        const size_t lds = state + sizeof(QvScratch);                   // width 13: 128 KiB + 1.2 KiB of the 160 KiB
        const int groups = 1 << (n_qubits - 2);
        const unsigned threads = (unsigned)(groups < 1024 ? groups : 1024);
        const unsigned grid = (unsigned)(B < 256 * 16 ? B : 256 * 16);
        if (lds > 64 * 1024)                                             // widths 12 and 13; below, the default limit holds
            FBX_HIP(hipFuncSetAttribute((const void*)qv_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(qv_block_kernel, dim3(grid), dim3(threads), lds, stream(), n_qubits, (long long)B, L, d_pairs, d_gates,
                           d_probs_out, d_median_out, (unsigned long long*)d_heavy_mask_out, d_heavy_prob_out, d_heavy_count_out);
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_qv_heavy_outputs(int n_qubits, int64_t B, int L, const uint8_t* pairs, const double* gates, double* probs_out,
                         double* median_out, uint64_t* heavy_mask_out, double* heavy_prob_out, int32_t* heavy_count_out) {
    FBX_TRY(qv_heavy_outputs_check(n_qubits, B, L, pairs, gates, probs_out, median_out, heavy_mask_out, heavy_prob_out, heavy_count_out));
    const size_t n_gates = (size_t)B * (size_t)L;
    for (size_t g = 0; g < n_gates; ++g)
        FBX_REQUIRE(pairs[2 * g] < n_qubits && pairs[2 * g + 1] < n_qubits && pairs[2 * g] != pairs[2 * g + 1],
                    "fbx_qv_heavy_outputs: a gate needs two different qubits below n_qubits");
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t n = (size_t)B, N = (size_t)1 << n_qubits, W = N >= 64 ? N / 64 : 1;
    HostIO io; uint8_t* dp; double *dg, *dprob, *dmed, *dhp; uint64_t* dmask; int32_t* dhc;
    FBX_TRY(io.in(pairs, 2 * n_gates, &dp)); FBX_TRY(io.in(gates, 32 * n_gates, &dg));
    FBX_TRY(io.out_opt(probs_out, n * N, &dprob)); FBX_TRY(io.out_opt(median_out, n, &dmed));
    FBX_TRY(io.out_opt(heavy_mask_out, n * W, &dmask)); FBX_TRY(io.out_opt(heavy_prob_out, n, &dhp));
    FBX_TRY(io.out_opt(heavy_count_out, n, &dhc));
    FBX_TRY(fbx_qv_heavy_outputs_dev(n_qubits, B, L, dp, dg, dprob, dmed, dmask, dhp, dhc));
    return io.finish();
}

int fbx_qv_count_heavy_dev(int n_qubits, int64_t B, int64_t n_shots, const uint8_t* d_bits, const uint64_t* d_heavy_mask,
                           int64_t* d_counts_out) {
    FBX_TRY(qv_count_heavy_check(n_qubits, B, n_shots, d_bits, d_heavy_mask, d_counts_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    switch (n_qubits) {
#define FBX_QV_COUNT(NQ) case NQ: return launch_qv_count<NQ>(B, n_shots, d_bits, d_heavy_mask, d_counts_out)
        FBX_QV_COUNT(2); FBX_QV_COUNT(3); FBX_QV_COUNT(4); FBX_QV_COUNT(5); FBX_QV_COUNT(6); FBX_QV_COUNT(7); FBX_QV_COUNT(8);
        FBX_QV_COUNT(9); FBX_QV_COUNT(10); FBX_QV_COUNT(11); FBX_QV_COUNT(12); FBX_QV_COUNT(13);
#undef FBX_QV_COUNT
    }
    return FBX_ERR_UNSUPPORTED;
}

int fbx_qv_count_heavy(int n_qubits, int64_t B, int64_t n_shots, const uint8_t* bits, const uint64_t* heavy_mask,
                       int64_t* counts_out) {
    FBX_TRY(qv_count_heavy_check(n_qubits, B, n_shots, bits, heavy_mask, counts_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t N = (size_t)1 << n_qubits, W = N >= 64 ? N / 64 : 1;
    HostIO io; uint8_t* db; uint64_t* dm; int64_t* dc;
    FBX_TRY(io.in(bits, (size_t)B * n_shots * n_qubits, &db)); FBX_TRY(io.in(heavy_mask, (size_t)B * W, &dm));
    FBX_TRY(io.out(counts_out, (size_t)B, &dc));
    FBX_TRY(fbx_qv_count_heavy_dev(n_qubits, B, n_shots, db, dm, dc));
    return io.finish();
}

}  // namespace fbx C ABI
