// fbx_sample_wide.hip -- fbx_sample_bitstrings_wide: measured bitstrings for widths 14..26, where the fp64 table of prefix sums of an
// item (8 B x 2^n) no longer fits the LDS of a CU and lives in device memory (the WS_SAMPLE_WIDE workspace).  The stream, the
// layouts and the poisoned-item rule are those of fbx_sample.hip (include/fbx.h); DESIGN.md 4.17 has the arguments in full.
//
// Six launches per chunk of items, N = 2^n entries cut into blocks of 4096:
//   1 totals   (block, item)  the block's sum of p in one fixed order; a weight that is negative or not finite flags the item
//   2 state    item           T = the block sums in order; lambda, the flips, T checked; status_out; keep = 1 - lambda, lambda T / N
//   3 scan     (block, item)  w from p, the inclusive prefix sums of the block on the scheme of sample_build_table (a thread's
//                             chunk in order, the lanes chained with readlane, the wavefronts chained through LDS), the block's last
//                             entry as its total, the last index of positive weight
//   4 offsets  item           the block totals scanned on the same scheme one level up: lane l owns a run of consecutive blocks and
//                             chains o_{j+1} = fl(o_j + total) through it, the lanes chain O_{l+1} = fl(O_l + run total_l)
//   5 apply    (block, item)  C_i = fl(O_l + fl(o_j + local_i)) in place
//   6 draw     (item, shot range)  a coarse table S[j] = C[(j + 1) R - 1], R = N / 4096, in LDS: 12 LDS steps to the segment, n - 12
//                             dependent reads of the table inside it, the flips, the bytes staged in LDS and stored as 16-byte vectors
//
// The table is non-decreasing by construction, seams included.  Inside a block local_i is (sample_build_table's argument), and
// x -> fl(O + fl(o + x)) does not decrease.  Between block k and its successor in the same lane's run: the last entry of k is
// fl(O_l + fl(o_j + total_k)) = fl(O_l + o_{j+1}), and the first of k + 1 is fl(O_l + fl(o_{j+1} + local_0)) >= that, equal when
// w = 0 (local_0 = 0).  Between the last block of lane l and the first of lane l + 1: fl(O_l + run total_l) = O_{l+1} against
// fl(O_{l+1} + fl(0 + local_0)) >= O_{l+1}.  (A flat C_i = fl(O_k + local_i) with O_k from the same lane-parallel scan would NOT have
// this property: fl(fl(O + o_j) + total) and fl(O + fl(o_j + total)) may differ by an ulp in either direction.)  No sum uses an atomic;
// the order of every one of them depends on the width alone.
#include "fbx_sample_common.hpp"
#include <algorithm>

namespace fbx {

constexpr int SW_MIN_WIDTH = 14, SW_MAX_WIDTH = 26;
constexpr int SW_THREADS = 512;
constexpr int SW_BLOCK = 4096;                   // entries per block of the table
constexpr int SW_E = SW_BLOCK / SW_THREADS;      // consecutive entries per thread in the totals and the scan
constexpr int SW_COARSE = 4096;                  // entries of the coarse table of the draw
constexpr int64_t SW_MAX_CHUNK = 32768;          // items per chunk (grid.y)

struct SwState {                                 // one per item of the chunk, zeroed in front of pass 1
    double keep, upart, total;                   // 1 - lambda, lambda T / N, C_{N-1}
    double flip[2 * SW_MAX_WIDTH];
    int lastpos1;                                // 1 + the last index of positive weight (0: none yet)
    unsigned bad;                                // pass 1: a weight that is negative or not finite
    int good;                                    // pass 2: the item can be sampled
    int lam_zero;
};

// ---------------------------------------------------------------------------------------------------- 1 totals
__global__ void __launch_bounds__(SW_THREADS)
sw_totals_kernel(int n, const double* __restrict__ probs, double* __restrict__ part, SwState* __restrict__ st) {
    __shared__ double red[SW_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const size_t N = (size_t)1 << n, nblk = N / SW_BLOCK, item = blockIdx.y, blk = blockIdx.x;
    const double* p = probs + item * N + blk * SW_BLOCK + (size_t)tid * SW_E;
    double local = 0.0;
    unsigned bad = 0;
#pragma unroll
    for (int e = 0; e < SW_E; ++e) {
        const double v = p[e];
        if (!(v >= 0.0 && v < __builtin_inf())) bad = 1;
        local += v;
    }
    double s = wave_sum(local);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        s = 0.0;
#pragma unroll
        for (int k = 0; k < SW_THREADS / 64; ++k) s += red[k];
        part[item * nblk + blk] = s;
    }
    if (__any(bad) && (tid & 63) == 0) atomicOr(&st[item].bad, 1u);
}

// ---------------------------------------------------------------------------------------------------- 2 state
__global__ void __launch_bounds__(64)
sw_state_kernel(int n, long long item0, const double* __restrict__ part, const double* __restrict__ depolarizing,
                const double* __restrict__ readout_flip, SwState* __restrict__ st, int* __restrict__ status_out) {
    const int lane = (int)threadIdx.x;
    const size_t N = (size_t)1 << n, nblk = N / SW_BLOCK, item = blockIdx.x;
    const int run = nblk >= 64 ? (int)(nblk / 64) : 1;
    const double* pp = part + item * nblk;
    double local = 0.0;
    for (int j = 0; j < run; ++j) {
        const size_t k = (size_t)lane * run + j;
        if (k < nblk) local += pp[k];
    }
    const double T = wave_sum(local);                 // a lane's run in order, then the lanes: one fixed order per width
    SwState* s = st + item;
    unsigned bad = s->bad;
    if (!(T > 0.0 && T < __builtin_inf())) bad = 1;
    const double lam = depolarizing ? depolarizing[item0 + item] : 0.0;
    if (sample_bad_probability(lam)) bad = 1;
    if (readout_flip && lane < 2 * n) {
        const double f = readout_flip[(item0 + item) * 2 * n + lane];
        s->flip[lane] = f;
        if (sample_bad_probability(f)) bad = 1;
    }
    bad = __any(bad) ? 1u : 0u;
    if (lane == 0) {
        s->good = bad ? 0 : 1;
        s->lam_zero = lam == 0.0 ? 1 : 0;
        s->keep = 1.0 - lam;
        s->upart = lam * T * (1.0 / (double)N);
        if (status_out) status_out[item0 + item] = (int)bad;
    }
}

// ---------------------------------------------------------------------------------------------------- 3 scan
__global__ void __launch_bounds__(SW_THREADS)
sw_scan_kernel(int n, const double* __restrict__ probs, double* __restrict__ table, double* __restrict__ tot, SwState* __restrict__ st) {
    __shared__ double wtot[SW_THREADS / 64];
    __shared__ int lastpos;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t N = (size_t)1 << n, nblk = N / SW_BLOCK, item = blockIdx.y, blk = blockIdx.x;
    SwState* s = st + item;
    if (!s->good) return;                             // (the whole workgroup)
    if (tid == 0) lastpos = -1;
    const size_t first = blk * SW_BLOCK + (size_t)tid * SW_E;
    const double* p = probs + item * N + first;
    double w[SW_E];
#pragma unroll
    for (int e = 0; e < SW_E; ++e) w[e] = p[e];
    if (!s->lam_zero) {
        const double keep = s->keep, uniform_part = s->upart;
#pragma unroll
        for (int e = 0; e < SW_E; ++e) w[e] = keep * w[e] + uniform_part;
    }
    int last = -1;
    double run = 0.0;
#pragma unroll
    for (int e = 0; e < SW_E; ++e) {
        if (w[e] > 0.0) last = (int)first + e;
        run += w[e];
        w[e] = run;                                   // L_e
    }
    // the offsets of the lanes, one after the other (wave-uniform arithmetic: every lane follows the whole chain)
    double off = 0.0, chain = 0.0;
    for (int l = 0; l < 64; ++l) {
        if (lane == l) off = chain;
        chain += readlane_f64(run, l);
    }
    if (lane == 0) wtot[wave] = chain;
    __syncthreads();
    if (last >= 0) atomicMax(&lastpos, last);
    double woff = 0.0;
    for (int k = 0; k < wave; ++k) woff += wtot[k];
    double* c = table + item * N + first;
#pragma unroll
    for (int e = 0; e < SW_E; ++e) c[e] = woff + (off + w[e]);
    if (tid == SW_THREADS - 1) tot[item * nblk + blk] = woff + (off + w[SW_E - 1]);     // the block's last entry
    __syncthreads();
    if (tid == 0 && lastpos >= 0) atomicMax(&s->lastpos1, lastpos + 1);
}

// ---------------------------------------------------------------------------------------------------- 4 offsets
// block k = lane l's j-th (l = k / run, j = k % run): offB[k] = o_j, offA[k] = O_l
__global__ void __launch_bounds__(64)
sw_offsets_kernel(int n, const double* __restrict__ tot, double* __restrict__ offA, double* __restrict__ offB, SwState* __restrict__ st) {
    const int lane = (int)threadIdx.x;
    const size_t nblk = ((size_t)1 << n) / SW_BLOCK, item = blockIdx.x;
    SwState* s = st + item;
    if (!s->good) return;
    const int run = nblk >= 64 ? (int)(nblk / 64) : 1;
    const size_t k0 = (size_t)lane * run, base = item * nblk;
    double o = 0.0;
    for (int j = 0; j < run; ++j)
        if (k0 + j < nblk) { offB[base + k0 + j] = o; o += tot[base + k0 + j]; }
    double off = 0.0, chain = 0.0;
    for (int l = 0; l < 64; ++l) {
        if (lane == l) off = chain;
        chain += readlane_f64(o, l);
    }
    for (int j = 0; j < run; ++j)
        if (k0 + j < nblk) offA[base + k0 + j] = off;
    if (lane == 0) s->total = chain;                  // = C_{N-1}: fl(O_l + run total_l) of the last lane that owns blocks
}

// ---------------------------------------------------------------------------------------------------- 5 apply
__global__ void __launch_bounds__(SW_THREADS)
sw_apply_kernel(int n, double* __restrict__ table, const double* __restrict__ offA, const double* __restrict__ offB,
                const SwState* __restrict__ st) {
    const size_t N = (size_t)1 << n, nblk = N / SW_BLOCK, item = blockIdx.y, blk = blockIdx.x;
    if (!st[item].good) return;
    const double O = offA[item * nblk + blk], o = offB[item * nblk + blk];
    double2* c = reinterpret_cast<double2*>(table + item * N + blk * SW_BLOCK);        // 16-byte aligned: the workspace is ours
#pragma unroll
    for (int e = 0; e < SW_BLOCK / 2 / SW_THREADS; ++e) {
        double2 v = c[threadIdx.x + e * SW_THREADS];
        v.x = O + (o + v.x);
        v.y = O + (o + v.y);
        c[threadIdx.x + e * SW_THREADS] = v;
    }
}

// ---------------------------------------------------------------------------------------------------- 6 draw
extern __shared__ __attribute__((aligned(16))) unsigned char sw_lds[];
constexpr size_t SW_LDS_FLIP = sizeof(double) * SW_COARSE, SW_LDS_STAGE = SW_LDS_FLIP + sizeof(double) * 2 * SW_MAX_WIDTH;
static_assert(SW_LDS_STAGE % 16 == 0, "the staging area starts on a 16-byte boundary");
static size_t sw_draw_lds(int n) { return SW_LDS_STAGE + (size_t)SW_THREADS * n + 16; }

// The outcome of shot `shot` of the item with id (g0, g1), readout flips applied: n bits, qubit 0 the most significant.
__device__ __forceinline__ unsigned sw_draw(int n, const double* __restrict__ C, const double* S, const double* flip, double total,
                                            int lastpos, bool flips, uint32_t g0, uint32_t g1, uint32_t k0, uint32_t k1, uint32_t shot) {
    uint32_t c[4] = {g0, g1, shot, 0u};
    philox4x32_10(c, k0, k1);
    const unsigned long long k = ((unsigned long long)(c[0] >> 5) << 26) | (unsigned long long)(c[1] >> 6);
    const double t = ((double)k * 0x1p-53) * total;
    int pos = 0;                                      // how many coarse entries are <= t
#pragma unroll
    for (int step = SW_COARSE >> 1; step > 0; step >>= 1)
        if (S[pos + step - 1] <= t) pos += step;
    if (pos == SW_COARSE - 1 && S[SW_COARSE - 1] <= t) pos = SW_COARSE;
    unsigned idx;
    if (pos == SW_COARSE) {
        idx = (unsigned)lastpos;                      // rounding left no entry above t
    } else {                                          // the segment's last entry is > t: the first such entry among its R
        const int R = 1 << (n - 12);
        const double* seg = C + (size_t)pos * R;
        int q = 0;
        for (int step = R >> 1; step > 0; step >>= 1)
            if (seg[q + step - 1] <= t) q += step;
        idx = (unsigned)pos * (unsigned)R + (unsigned)q;
    }
    if (flips) {
        const int blocks = (2 + n + 3) / 4;
        unsigned mask = 0;
        for (int b = 0; b < blocks; ++b) {
            if (b > 0) { c[0] = g0; c[1] = g1; c[2] = shot; c[3] = (uint32_t)b; philox4x32_10(c, k0, k1); }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int j = 4 * b + x - 2;
                if (j >= 0 && j < n) {
                    const unsigned d = (idx >> (n - 1 - j)) & 1u;
                    if ((double)c[x] * 0x1p-32 < flip[2 * j + d]) mask |= 1u << (n - 1 - j);
                }
            }
        }
        idx ^= mask;
    }
    return idx;
}

// unit u = (item u / pieces, shot range u % pieces) of the chunk; a workgroup takes a unit, a tile of 512 shots at a time
__global__ void __launch_bounds__(SW_THREADS)
sw_draw_kernel(int n, long long items, long long n_shots, long long pieces, long long piece_shots, const double* __restrict__ table,
               const SwState* __restrict__ st, int flips, unsigned long long seed, long long first_id, uint8_t* __restrict__ bits) {
    double* S = reinterpret_cast<double*>(sw_lds);
    double* flip = reinterpret_cast<double*>(sw_lds + SW_LDS_FLIP);
    unsigned char* stage = sw_lds + SW_LDS_STAGE;
    const int tid = (int)threadIdx.x;
    const size_t N = (size_t)1 << n, R = N / SW_COARSE;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const long long units = items * pieces;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long b = u / pieces, piece = u - b * pieces;
        const long long s0 = piece * piece_shots, s1 = s0 + piece_shots < n_shots ? s0 + piece_shots : n_shots;
        const SwState* s = st + b;
        const bool good = s->good != 0;               // a poisoned item: zeros, and the table is never touched
        const double* C = table + (size_t)b * N;
        __syncthreads();                              // the previous unit is done with S and flip
        if (good) {
            for (int j = tid; j < SW_COARSE; j += SW_THREADS) S[j] = C[(size_t)(j + 1) * R - 1];
            if (flips && tid < 2 * n) flip[tid] = s->flip[tid];
        }
        const double total = s->total;
        const int lastpos = s->lastpos1 - 1;
        const unsigned long long g = (unsigned long long)(first_id + b);
        uint8_t* rec = bits + (size_t)b * (size_t)n_shots * n;
        __syncthreads();
        for (long long ts = s0; ts < s1; ts += SW_THREADS) {
            const int cnt = (int)(s1 - ts < SW_THREADS ? s1 - ts : SW_THREADS);
            uint8_t* out = rec + ts * n;
            const int mis = (int)((uintptr_t)out & 15);          // staged at the same offset mod 16 as in memory
            if (tid < cnt) {
                const unsigned idx = good ? sw_draw(n, C, S, flip, total, lastpos, flips != 0, (uint32_t)g, (uint32_t)(g >> 32), k0, k1,
                                                    (uint32_t)(ts + tid))
                                          : 0u;
                unsigned char* d = stage + mis + tid * n;
                for (int q = 0; q < n; ++q) d[q] = (unsigned char)((idx >> (n - 1 - q)) & 1u);
            }
            __syncthreads();
            // the bytes in front of the first 16-byte boundary and behind the last full vector go byte-wise
            const int nbytes = cnt * n;
            int head = mis ? 16 - mis : 0;
            head = head < nbytes ? head : nbytes;
            const int nvec = (nbytes - head) / 16, tail0 = head + 16 * nvec;
            const uint4* src = reinterpret_cast<const uint4*>(stage + mis + head);
            uint4* dst = reinterpret_cast<uint4*>(out + head);
            for (int v = tid; v < nvec; v += SW_THREADS) dst[v] = src[v];
            if (tid < head) out[tid] = stage[mis + tid];
            if (tail0 + tid < nbytes) out[tail0 + tid] = stage[mis + tail0 + tid];      // (fewer than 16 bytes)
            __syncthreads();                          // the staging area is reused by the next tile
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host
static int sw_check(int n_qubits, int64_t B, int64_t n_shots, const void* probs, int64_t first_item, const void* bits) {
    return sample_check("fbx_sample_bitstrings_wide", SW_MIN_WIDTH, SW_MAX_WIDTH,
                        "narrower tables belong to fbx_sample_bitstrings, wider ones are not built", n_qubits, B, n_shots, probs,
                        first_item, bits);
}

static int sw_run(int n, int64_t B, int64_t n_shots, const double* d_probs, const double* d_lam, const double* d_flip, uint64_t seed,
                  int64_t first_item, uint8_t* d_bits, int32_t* d_status) {
    const size_t N = (size_t)1 << n, nblk = N / SW_BLOCK;
    // the chunk: as many items as the workspace cap admits, at least one
    const size_t per = 8 * N + 4 * 8 * nblk + sizeof(SwState);
    const double cap = option_sample_wide_workspace_mib() * 1048576.0;
    int64_t chunk = (int64_t)(cap / (double)per);
    chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(chunk, B), SW_MAX_CHUNK));
    void* ws = nullptr;
    FBX_TRY(workspace(WS_SAMPLE_WIDE, per * (size_t)chunk, &ws));
    unsigned char* w = static_cast<unsigned char*>(ws);
    double* table = reinterpret_cast<double*>(w);          w += 8 * N * (size_t)chunk;
    double* part = reinterpret_cast<double*>(w);           w += 8 * nblk * (size_t)chunk;
    double* tot = reinterpret_cast<double*>(w);            w += 8 * nblk * (size_t)chunk;
    double* offA = reinterpret_cast<double*>(w);           w += 8 * nblk * (size_t)chunk;
    double* offB = reinterpret_cast<double*>(w);           w += 8 * nblk * (size_t)chunk;
    SwState* st = reinterpret_cast<SwState*>(w);
    const size_t lds = sw_draw_lds(n);
    for (int64_t item0 = 0; item0 < B; item0 += chunk) {
        const int64_t cb = std::min<int64_t>(chunk, B - item0);
        const double* probs = d_probs + (size_t)item0 * N;
        const dim3 grid((unsigned)nblk, (unsigned)cb);
        FBX_HIP(hipMemsetAsync(st, 0, sizeof(SwState) * (size_t)cb, stream()));
        hipLaunchKernelGGL(sw_totals_kernel, grid, dim3(SW_THREADS), 0, stream(), n, probs, part, st);
        hipLaunchKernelGGL(sw_state_kernel, dim3((unsigned)cb), dim3(64), 0, stream(), n, (long long)item0, part, d_lam, d_flip, st,
                           d_status);
        hipLaunchKernelGGL(sw_scan_kernel, grid, dim3(SW_THREADS), 0, stream(), n, probs, table, tot, st);
        hipLaunchKernelGGL(sw_offsets_kernel, dim3((unsigned)cb), dim3(64), 0, stream(), n, tot, offA, offB, st);
        hipLaunchKernelGGL(sw_apply_kernel, grid, dim3(SW_THREADS), 0, stream(), n, table, offA, offB, st);
        FBX_HIP(hipGetLastError());
        // A record is cut into shot ranges until there are a few units per CU (256 CUs), never below 16 shots per lane: whole
        // multiples of 16 shots, so that only the two ends of a record can be off a 16-byte boundary.
        constexpr int64_t WANTED_UNITS = 1024, MIN_PIECE = 16 * SW_THREADS;
        int64_t pieces = (WANTED_UNITS + cb - 1) / cb;
        const int64_t most = (n_shots + MIN_PIECE - 1) / MIN_PIECE;
        pieces = std::max<int64_t>(1, std::min(pieces, most));
        int64_t piece_shots = (n_shots + pieces - 1) / pieces;
        piece_shots = (piece_shots + 15) / 16 * 16;
        pieces = (n_shots + piece_shots - 1) / piece_shots;
        const int64_t units = cb * pieces;
        FBX_TRY(launch_lds(sw_draw_kernel, dim3((unsigned)std::min<int64_t>(units, 256 * 16)), dim3(SW_THREADS), lds, n, (long long)cb,
                           (long long)n_shots, (long long)pieces, (long long)piece_shots, (const double*)table, (const SwState*)st,
                           d_flip ? 1 : 0, (unsigned long long)seed, (long long)(first_item + item0),
                           d_bits + (size_t)item0 * (size_t)n_shots * n));
    }
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_sample_bitstrings_wide_dev(int n_qubits, int64_t B, int64_t n_shots, const double* d_probs, const double* d_depolarizing,
                                   const double* d_readout_flip, uint64_t seed, int64_t first_item, uint8_t* d_bits_out,
                                   int32_t* d_status_out) {
    FBX_TRY(sw_check(n_qubits, B, n_shots, d_probs, first_item, d_bits_out));
    FBX_TRY(ensure_device());
    if (B == 0 || n_shots == 0) return FBX_OK;
    return sw_run(n_qubits, B, n_shots, d_probs, d_depolarizing, d_readout_flip, seed, first_item, d_bits_out, d_status_out);
}

int fbx_sample_bitstrings_wide(int n_qubits, int64_t B, int64_t n_shots, const double* probs, const double* depolarizing,
                               const double* readout_flip, uint64_t seed, int64_t first_item, uint8_t* bits_out,
                               int32_t* status_out) {
    FBX_TRY(sw_check(n_qubits, B, n_shots, probs, first_item, bits_out));
    FBX_TRY(ensure_device());
    if (B == 0 || n_shots == 0) return FBX_OK;
    const size_t n = (size_t)B, N = (size_t)1 << n_qubits;
    HostIO io; double *dp, *dl = nullptr, *df = nullptr; uint8_t* db; int32_t* ds;
    FBX_TRY(io.in(probs, n * N, &dp));
    if (depolarizing) FBX_TRY(io.in(depolarizing, n, &dl));
    if (readout_flip) FBX_TRY(io.in(readout_flip, n * 2 * (size_t)n_qubits, &df));
    FBX_TRY(io.out(bits_out, n * (size_t)n_shots * (size_t)n_qubits, &db));
    FBX_TRY(io.out_opt(status_out, n, &ds));
    FBX_TRY(fbx_sample_bitstrings_wide_dev(n_qubits, B, n_shots, dp, dl, df, seed, first_item, db, ds));
    return io.finish();
}

}  // fbx C ABI
