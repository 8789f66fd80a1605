// fbx_sample.hip -- measured bitstrings drawn from outcome distributions (fbx_sample_bitstrings): the step between the ideal
// distributions of fbx_qv_heavy_outputs and the bit records that fbx_qv_count_heavy, fbx_shots_to_moments and fbx_bit_histogram read.
//
// A team (a wavefront for widths 1..8, four per workgroup and no workgroup barrier; a workgroup of 512 threads for widths 9..13)
// holds the inclusive prefix sums C of one item's weights in LDS (width 13: 64 KiB, two workgroups per CU) and draws a range of
// the item's shots from them.  A record is cut into shot ranges when the batch alone would not fill the chip; the stream of
// include/fbx.h (a shot owns the Philox blocks with counter (item id, shot, t)) makes a shot independent of who draws it, and every
// team of an item rebuilds the same table: the order of every sum below depends on the width alone.
//
// The table is non-decreasing by construction, so the search can never stop at an outcome of weight zero: a thread sums its own
// chunk of consecutive entries in order (L), the lanes of a wavefront get their offsets o one after the other -- o_{l+1} = fl(o_l +
// total_l), which IS the rounded last entry of lane l -- the wavefronts of a workgroup theirs (O) in the same way, and entry e of
// lane l of wavefront w is fl(O_w + fl(o_l + L_e)): a non-decreasing function of a non-decreasing sequence inside a chunk, and at
// every seam the next chunk starts from the very number the previous one ended on.  An entry of weight zero repeats its
// predecessor exactly; "the smallest i with C_i > t" is then never such an entry.
//
// Per shot: one Philox block for the draw (53 bits of its first two words), the dependent LDS reads of the search (log2(N) of them
// for widths 1..8; from width 9 on a bucket table indexed by the top bits of the draw narrows the range first), and for
// readout flips the words 2 .. 2 + n - 1 of the shot's blocks (up to three more).  Stores mirror the read side of qv_count_record: a
// lane draws a run of 16 shots -- 16 bits of outcome each, shifted through four 64-bit registers -- expands them into 16 n bytes and
// writes them as n 16-byte vectors; the shots in front of the first 16-byte boundary of a range and behind its last full run go
// byte-wise.
#include "fbx_sample_common.hpp"

namespace fbx {

constexpr int SAMPLE_BLOCK_THREADS = 512;       // widths 9..13
constexpr int SAMPLE_MAX_WIDTH = 13;
#ifndef FBX_SAMPLE_BUCKET_MIN_WIDTH
#define FBX_SAMPLE_BUCKET_MIN_WIDTH 9            // widths from here on shorten the search with the bucket table (14: never)
#endif

// Buckets of the draw (widths 9..13): bucket j holds the draws with j / K <= u < (j + 1) / K, K = N / 4, i.e. j = the top n - 2 bits
// of k.  t = fl(u C_{N-1}) does not decrease with u, and neither does the number of entries <= t with t, so with P[j] = the number
// of entries <= fl((j / K) C_{N-1}) and P[K] = N the answer for every draw of bucket j lies in P[j] .. P[j + 1]: the search runs over
// that range only and ends on the very entry the full search ends on.
template <int NQ> struct SampleBuckets {
    static constexpr bool on = NQ >= FBX_SAMPLE_BUCKET_MIN_WIDTH;
    static constexpr int bits = NQ > 2 ? NQ - 2 : 1, K = 1 << bits;
    static constexpr size_t bytes = on ? (sizeof(uint16_t) * (K + 1) + 7) / 8 * 8 : 0;
};

struct SampleScratch {
    double flip[2 * SAMPLE_MAX_WIDTH];          // the item's readout_flip [n][2]
    double red[SAMPLE_BLOCK_THREADS / 64];      // wavefront sums of the weights
    double wtot[SAMPLE_BLOCK_THREADS / 64];     // wavefront totals of the prefix sums
    int lastpos;                                // the last outcome of positive weight
    unsigned bad;
};

// LDS of one team: the prefix sums, the bucket table, the scratch
template <int NQ> constexpr size_t sample_team_bytes() {
    return sizeof(double) * ((size_t)1 << NQ) + SampleBuckets<NQ>::bytes + sizeof(SampleScratch);
}

template <bool WAVE>
__device__ __forceinline__ void sample_sync() {
    if constexpr (WAVE) FBX_WAVE_SYNC(); else __syncthreads();
}

// how many of the N entries are <= t (0..N) = the smallest i with C_i > t: log2(N) dependent reads, no branch
template <int NQ>
__device__ __forceinline__ int sample_count_le(const double* C, double t) {
    constexpr int N = 1 << NQ;
    int pos = 0;
#pragma unroll
    for (int step = N >> 1; step > 0; step >>= 1)
        if (C[pos + step - 1] <= t) pos += step;
    if (pos == N - 1 && C[N - 1] <= t) pos = N;
    return pos;
}

// The team's table of item `p` (its N weights); false for a poisoned item.  Every thread of the team calls it.
template <int NQ, bool WAVE>
__device__ bool sample_build_table(const double* __restrict__ p, const double* __restrict__ lam_ptr, const double* __restrict__ flip,
                                   double* C, uint16_t* P, SampleScratch* sc, int tid) {
    constexpr int N = 1 << NQ, NTH = WAVE ? 64 : SAMPLE_BLOCK_THREADS, E = N / NTH > 0 ? N / NTH : 1;
    const int lane = tid & 63;
    if (tid == 0) { sc->lastpos = -1; sc->bad = 0; }
    sample_sync<WAVE>();
    const bool owner = tid * E < N;              // (widths below 6: the lanes past N own nothing)
    double w[E];
    double local = 0.0;
    unsigned bad = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        w[e] = owner ? p[tid * E + e] : 0.0;
        if (!(w[e] >= 0.0 && w[e] < __builtin_inf())) bad = 1;
        local += w[e];
    }
    const double lam = lam_ptr ? *lam_ptr : 0.0;
    if (sample_bad_probability(lam)) bad = 1;
    if (flip && tid < 2 * NQ) {
        const double f = flip[tid];
        sc->flip[tid] = f;
        if (sample_bad_probability(f)) bad = 1;
    }
    // T: lanes (wave_sum), then wavefronts in order -- one fixed order per width
    double T = wave_sum(local);
    if constexpr (!WAVE) {
        if (lane == 0) sc->red[tid >> 6] = T;
        __syncthreads();
        T = 0.0;
#pragma unroll
        for (int k = 0; k < NTH / 64; ++k) T += sc->red[k];
    }
    if (!(T > 0.0 && T < __builtin_inf())) bad = 1;
    if (bad) atomicOr(&sc->bad, 1u);
    sample_sync<WAVE>();
    if (sc->bad) return false;
    if (lam != 0.0) {
        const double keep = 1.0 - lam, uniform_part = lam * T * (1.0 / N);
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = keep * w[e] + uniform_part;
    }
    int last = -1;
    double run = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (owner && w[e] > 0.0) last = tid * E + e;
        run += w[e];
        w[e] = run;                               // L_e
    }
    if (last >= 0) atomicMax(&sc->lastpos, last);
    // the offsets of the lanes, one after the other (wave-uniform arithmetic: every lane follows the whole chain)
    double off = 0.0, chain = 0.0;
    for (int l = 0; l < 64; ++l) {
        if (lane == l) off = chain;
        chain += readlane_f64(run, l);
    }
    double woff = 0.0;
    if constexpr (!WAVE) {
        const int wave = tid >> 6;
        if (lane == 0) sc->wtot[wave] = chain;
        __syncthreads();
        for (int k = 0; k < wave; ++k) woff += sc->wtot[k];
    }
    if (owner) {
#pragma unroll
        for (int e = 0; e < E; ++e) C[tid * E + e] = woff + (off + w[e]);
    }
    sample_sync<WAVE>();
    if constexpr (SampleBuckets<NQ>::on) {
        constexpr int K = SampleBuckets<NQ>::K;
        const double total = C[N - 1];
        for (int j = tid; j <= K; j += NTH)
            P[j] = j < K ? (uint16_t)sample_count_le<NQ>(C, ((double)j * (1.0 / K)) * total) : (uint16_t)N;
        sample_sync<WAVE>();
    }
    return true;
}

// The outcome of shot `s` of the item with id (g0, g1), readout flips applied: NQ bits, qubit 0 the most significant.
template <int NQ>
__device__ __forceinline__ unsigned sample_draw(const double* C, const uint16_t* P, const SampleScratch* sc, double total, bool flips,
                                                uint32_t g0, uint32_t g1, uint32_t k0, uint32_t k1, uint32_t s) {
    constexpr int N = 1 << NQ;
    uint32_t c[4] = {g0, g1, s, 0u};
    philox4x32_10(c, k0, k1);
    const unsigned long long k = ((unsigned long long)(c[0] >> 5) << 26) | (unsigned long long)(c[1] >> 6);
    const double t = ((double)k * 0x1p-53) * total;
    int pos;
    if constexpr (SampleBuckets<NQ>::on) {
        const int j = (int)(k >> (53 - SampleBuckets<NQ>::bits));
        int hi = P[j + 1];
        pos = P[j];
        while (pos < hi) {                        // the first entry > t among pos .. hi - 1, or hi
            const int mid = (pos + hi) >> 1;
            if (C[mid] <= t) pos = mid + 1; else hi = mid;
        }
    } else {
        pos = sample_count_le<NQ>(C, t);
    }
    if (pos == N) pos = sc->lastpos;              // rounding left no entry above t
    unsigned idx = (unsigned)pos;
    if (flips) {
        constexpr int BLOCKS = (2 + NQ + 3) / 4;
        unsigned mask = 0;
#pragma unroll
        for (int b = 0; b < BLOCKS; ++b) {
            if (b > 0) { c[0] = g0; c[1] = g1; c[2] = s; c[3] = (uint32_t)b; philox4x32_10(c, k0, k1); }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int j = 4 * b + x - 2;
                if (j >= 0 && j < NQ) {
                    const unsigned d = (idx >> (NQ - 1 - j)) & 1u;
                    if ((double)c[x] * 0x1p-32 < sc->flip[2 * j + d]) mask |= 1u << (NQ - 1 - j);
                }
            }
        }
        idx ^= mask;
    }
    return idx;
}

// Shots s0 .. s1 - 1 of the record `rec` by one team; `good` false: zeros.
template <int NQ, bool WAVE>
__device__ void sample_range(uint8_t* __restrict__ rec, long long s0, long long s1, bool good, const double* C, const uint16_t* P,
                             const SampleScratch* sc,
                             bool flips, uint32_t g0, uint32_t g1, uint32_t k0, uint32_t k1, int tid) {
    constexpr int NTH = WAVE ? 64 : SAMPLE_BLOCK_THREADS;
    const double total = good ? C[(1 << NQ) - 1] : 0.0;
    // runs of 16 shots = NQ 16-byte vectors per lane, from the first shot of the range that starts on a 16-byte boundary
    long long head = s1;
    for (int k = 0; k < 16 && s0 + k < s1; ++k)
        if ((((uintptr_t)rec + (uintptr_t)((s0 + k) * NQ)) & 15) == 0) { head = s0 + k; break; }
    const long long runs = (s1 - head) / 16;
    for (long long r = tid; r < runs; r += NTH) {
        const long long first = head + 16 * r;
        unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;          // shot j of the run ends up in bits 16 j .. 16 j + 15
        if (good) {
#pragma unroll 1
            for (int j = 0; j < 16; ++j) {
                const unsigned long long idx = sample_draw<NQ>(C, P, sc, total, flips, g0, g1, k0, k1, (uint32_t)(first + j));
                a0 = (a0 >> 16) | (a1 << 48); a1 = (a1 >> 16) | (a2 << 48); a2 = (a2 >> 16) | (a3 << 48); a3 = (a3 >> 16) | (idx << 48);
            }
        }
        const unsigned long long a[4] = {a0, a1, a2, a3};
        unsigned long long x[2 * NQ];
#pragma unroll
        for (int v = 0; v < 2 * NQ; ++v) x[v] = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int byte = j * NQ + q;
                x[byte >> 3] |= ((a[j >> 2] >> (16 * (j & 3) + (NQ - 1 - q))) & 1ull) << (8 * (byte & 7));
            }
        }
        ulonglong2* v = reinterpret_cast<ulonglong2*>(rec + first * NQ);
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = ulonglong2{x[2 * q], x[2 * q + 1]};
    }
    const long long tail0 = head + runs * 16, front = head - s0, rest = front + (s1 - tail0);
    for (long long k = tid; k < rest; k += NTH) {
        const long long s = k < front ? s0 + k : tail0 + (k - front);
        const unsigned idx = good ? sample_draw<NQ>(C, P, sc, total, flips, g0, g1, k0, k1, (uint32_t)s) : 0u;
#pragma unroll
        for (int q = 0; q < NQ; ++q) rec[s * NQ + q] = (uint8_t)((idx >> (NQ - 1 - q)) & 1u);
    }
}

extern __shared__ __attribute__((aligned(16))) unsigned char sample_lds[];

// unit u = (item u / pieces, shot range u % pieces); a wavefront (NQ <= 8, four per workgroup) or the workgroup takes a unit
template <int NQ>
__global__ void __launch_bounds__(NQ <= 8 ? 256 : SAMPLE_BLOCK_THREADS)
sample_kernel(long long B, long long n_shots, long long pieces, long long piece_shots, const double* __restrict__ probs,
              const double* __restrict__ depolarizing, const double* __restrict__ readout_flip, unsigned long long seed,
              long long first_item, uint8_t* __restrict__ bits_out, int* __restrict__ status_out) {
    constexpr bool WAVE = NQ <= 8;
    constexpr int N = 1 << NQ, TEAMS = WAVE ? 4 : 1;
    constexpr size_t PER_TEAM = sample_team_bytes<NQ>();
    const int team = WAVE ? uniform((int)(threadIdx.x >> 6)) : 0;
    const int tid = WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    double* C = reinterpret_cast<double*>(sample_lds + PER_TEAM * team);
    uint16_t* P = reinterpret_cast<uint16_t*>(sample_lds + PER_TEAM * team + sizeof(double) * N);
    SampleScratch* sc = reinterpret_cast<SampleScratch*>(sample_lds + PER_TEAM * team + sizeof(double) * N + SampleBuckets<NQ>::bytes);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const long long units = B * pieces;
    for (long long u = (long long)blockIdx.x * TEAMS + team; u < units; u += (long long)gridDim.x * TEAMS) {
        const long long b = u / pieces, piece = u - b * pieces;
        const long long s0 = piece * piece_shots, s1 = s0 + piece_shots < n_shots ? s0 + piece_shots : n_shots;
        const unsigned long long g = (unsigned long long)(first_item + b);
        const bool good = sample_build_table<NQ, WAVE>(probs + b * N, depolarizing ? depolarizing + b : nullptr,
                                                       readout_flip ? readout_flip + b * 2 * NQ : nullptr, C, P, sc, tid);
        if (piece == 0 && tid == 0 && status_out) status_out[b] = good ? 0 : 1;
        if (s0 < s1)
            sample_range<NQ, WAVE>(bits_out + b * n_shots * NQ, s0, s1, good, C, P, sc, readout_flip != nullptr, (uint32_t)g,
                                   (uint32_t)(g >> 32), k0, k1, tid);
        sample_sync<WAVE>();                      // the table and the scratch are reused by the team's next unit
    }
}

template <int NQ>
static int launch_sample(int64_t B, int64_t n_shots, const double* probs, const double* depolarizing, const double* readout_flip,
                         uint64_t seed, int64_t first_item, uint8_t* bits, int32_t* status) {
    constexpr bool WAVE = NQ <= 8;
    constexpr int TEAMS = WAVE ? 4 : 1, NTH = WAVE ? 64 : SAMPLE_BLOCK_THREADS;
    constexpr size_t lds = TEAMS * sample_team_bytes<NQ>();
    // A record is cut into shot ranges until there are a few units per CU (256 CUs), never below one run of 16 shots per lane:
    // whole multiples of 16 shots, so that only the two ends of a record are written byte-wise.
    constexpr int64_t WANTED_UNITS = 1024 * TEAMS, MIN_PIECE = 16 * NTH;
    int64_t pieces = (WANTED_UNITS + B - 1) / B;
    const int64_t most = (n_shots + MIN_PIECE - 1) / MIN_PIECE;
    pieces = pieces < most ? pieces : most;
    pieces = pieces < 1 ? 1 : pieces;
    int64_t piece_shots = (n_shots + pieces - 1) / pieces;
    piece_shots = (piece_shots + 15) / 16 * 16;
    pieces = (n_shots + piece_shots - 1) / piece_shots;
    const int64_t groups = (B * pieces + TEAMS - 1) / TEAMS;
    const unsigned grid = (unsigned)(groups < 256 * 16 ? groups : 256 * 16);
    if (lds > 64 * 1024)                          // width 13; below, the default limit holds
        FBX_HIP(hipFuncSetAttribute((const void*)sample_kernel<NQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(sample_kernel<NQ>, dim3(grid), dim3(WAVE ? 256 : SAMPLE_BLOCK_THREADS), lds, stream(), (long long)B,
                       (long long)n_shots, (long long)pieces, (long long)piece_shots, probs, depolarizing, readout_flip,
                       (unsigned long long)seed, (long long)first_item, bits, status);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

static int sample_check(int n_qubits, int64_t B, int64_t n_shots, const void* probs, int64_t first_item, const void* bits) {
    return sample_check("fbx_sample_bitstrings", 1, SAMPLE_MAX_WIDTH, "a wider table does not fit the LDS of one CU", n_qubits, B, n_shots,
                        probs, first_item, bits);
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_sample_bitstrings_dev(int n_qubits, int64_t B, int64_t n_shots, const double* d_probs, const double* d_depolarizing,
                              const double* d_readout_flip, uint64_t seed, int64_t first_item, uint8_t* d_bits_out,
                              int32_t* d_status_out) {
    FBX_TRY(sample_check(n_qubits, B, n_shots, d_probs, first_item, d_bits_out));
    FBX_TRY(ensure_device());
    if (B == 0 || n_shots == 0) return FBX_OK;
    switch (n_qubits) {
#define FBX_SAMPLE(NQ) case NQ: return launch_sample<NQ>(B, n_shots, d_probs, d_depolarizing, d_readout_flip, seed, first_item, \
                                                         d_bits_out, d_status_out)
        FBX_SAMPLE(1); FBX_SAMPLE(2); FBX_SAMPLE(3); FBX_SAMPLE(4); FBX_SAMPLE(5); FBX_SAMPLE(6); FBX_SAMPLE(7); FBX_SAMPLE(8);
        FBX_SAMPLE(9); FBX_SAMPLE(10); FBX_SAMPLE(11); FBX_SAMPLE(12); FBX_SAMPLE(13);
#undef FBX_SAMPLE
    }
    return FBX_ERR_UNSUPPORTED;
}

int fbx_sample_bitstrings(int n_qubits, int64_t B, int64_t n_shots, const double* probs, const double* depolarizing,
                          const double* readout_flip, uint64_t seed, int64_t first_item, uint8_t* bits_out, int32_t* status_out) {
    FBX_TRY(sample_check(n_qubits, B, n_shots, probs, first_item, bits_out));
    FBX_TRY(ensure_device());
    if (B == 0 || n_shots == 0) return FBX_OK;
    const size_t n = (size_t)B, N = (size_t)1 << n_qubits;
    HostIO io; double *dp, *dl = nullptr, *df = nullptr; uint8_t* db; int32_t* ds;
    FBX_TRY(io.in(probs, n * N, &dp));
    if (depolarizing) FBX_TRY(io.in(depolarizing, n, &dl));
    if (readout_flip) FBX_TRY(io.in(readout_flip, n * 2 * (size_t)n_qubits, &df));
    FBX_TRY(io.out(bits_out, n * (size_t)n_shots * (size_t)n_qubits, &db));
    FBX_TRY(io.out_opt(status_out, n, &ds));
    FBX_TRY(fbx_sample_bitstrings_dev(n_qubits, B, n_shots, dp, dl, df, seed, first_item, db, ds));
    return io.finish();
}

}  // fbx C ABI
