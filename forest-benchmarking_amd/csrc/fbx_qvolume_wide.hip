// fbx_qvolume_wide.hip -- quantum-volume heavy outputs and heavy-hitter counts for widths 14..26: the state of a
// circuit lives in HBM (16 B x 2^n in the WS_QV_WIDE workspace) and is worked on in LDS a tile at a time.
//
// Passes.  A circuit is cut into passes by qvw_plan_circuit (one lane per circuit on the device; the same function runs on the
// host where the pairs are host memory).  A pass names tile_bits LOCAL index bits, among them always the three lowest, and holds
// the longest run of consecutive gates whose targets are all local.  For a pass, workgroup (tile, circuit) owns the 2^tile_bits
// amplitudes whose other index bits spell the tile number: it gathers them into LDS (runs of at least 8 amplitudes = 128 B are
// contiguous in HBM), applies the gates of the pass there with the gate step of the narrow simulator (fbx_qv_gate.hpp, on the
// local index, swizzled by qv_slot) and writes the tile back.  One launch per pass over (tiles) x (circuits of the chunk); passes
// are ordered by the stream.  The first pass starts from |0...0> without a read.  A circuit with fewer passes than were launched
// leaves the surplus launches at once.
//
// After the last pass: probabilities (8 B x 2^n, in probs_out or in the workspace), smallest / largest bit pattern and the
// non-finite flag; the most-significant-digit radix select of fbx_qvolume.hip spread over workgroups (per round every workgroup
// adds a 256-bin LDS histogram to the circuit's global one with integer atomics, then one wavefront per circuit picks the digit;
// eight rounds cover 64 bits, finished circuits skip); the "count <= v1, smallest above" pass for rank N/2; the masks by
// __ballot with heavy_prob summed per block of QVW_BLOCK outputs and the blocks added in order by one workgroup per circuit.
// Nothing here waits for the host: the number of launches is a function of (n, L, tile_bits) in the _dev form and the planned
// maximum in the host-pointer form, and the results do not depend on it.
#include <algorithm>
#include <atomic>
#include "fbx_common.hpp"
#include "fbx_qv_gate.hpp"

namespace fbx {

constexpr int QVW_MIN_WIDTH = 14, QVW_MAX_WIDTH = 26;
constexpr int QVW_MIN_TILE = 8, QVW_MAX_TILE = 13, QVW_DEFAULT_TILE = 13;
constexpr int QVW_LOW_BITS = 3;                  // always local: 2^3 amplitudes x 16 B = 128 B contiguous
constexpr int QVW_BLOCK = 4096;                  // outputs per workgroup of the passes over the probabilities (256 threads x 16)
constexpr int QVW_MAX_CHUNK = 32768;             // circuits per launch (grid y)

// Greedy plan of one circuit: first[k] = first gate of pass k (first[n_passes .. L] = L), mask[k] = its local index bits
// (mask[n_passes .. L-1] = 0).  A pass takes gates while the targets not yet local still fit (each new target takes one of the
// tile_bits - 3 free places); the places then left are filled with the lowest index bits not yet local, which lengthens the
// contiguous runs of the tile in HBM.  Returns the number of passes, or -1 when a pair is not two different qubits below n.
__host__ __device__ inline int qvw_plan_circuit(int n, int L, int T, const uint8_t* pairs, int32_t* first, uint32_t* mask) {
    bool ok = true;
    for (int l = 0; l < L; ++l) ok = ok && pairs[2 * l] < n && pairs[2 * l + 1] < n && pairs[2 * l] != pairs[2 * l + 1];
    int np = 0, l = 0;
    while (ok && l < L) {
        uint32_t m = (1u << QVW_LOW_BITS) - 1u;
        int cnt = QVW_LOW_BITS;
        first[np] = l;
        while (l < L) {
            const uint32_t b0 = 1u << (n - 1 - pairs[2 * l]), b1 = 1u << (n - 1 - pairs[2 * l + 1]);
            const int add = ((m & b0) ? 0 : 1) + ((m & b1) ? 0 : 1);
            if (cnt + add > T) break;
            m |= b0 | b1; cnt += add; ++l;
        }
        for (int b = QVW_LOW_BITS; cnt < T; ++b)
            if (!((m >> b) & 1u)) { m |= 1u << b; ++cnt; }
        mask[np++] = m;
    }
    for (int k = np; k <= L; ++k) first[k] = L;
    for (int k = np; k < L; ++k) mask[k] = 0u;
    return ok ? np : -1;
}

// launches that cover every circuit of L gates: a pass that is not the last holds at least (T - 3) / 2 gates
static int qvw_pass_bound(int L, int T) {
    const int per = (T - QVW_LOW_BITS) / 2;
    return (L + per - 1) / per;
}

__global__ void __launch_bounds__(256)
qvw_plan_kernel(int n, long long B, int L, int T, const uint8_t* __restrict__ pairs, int32_t* __restrict__ npass,
                int32_t* __restrict__ first, uint32_t* __restrict__ mask) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) npass[b] = qvw_plan_circuit(n, L, T, pairs + (size_t)b * L * 2, first + (size_t)b * (L + 1), mask + (size_t)b * L);
}

// bits of v, lowest first, placed on the set bits of m from its `skip`-th on
__device__ __forceinline__ unsigned qvw_deposit(unsigned v, unsigned m, int skip) {
    for (int s = 0; s < skip; ++s) m &= m - 1u;
    unsigned out = 0;
    while (v) {
        if (v & 1u) out |= m & (0u - m);
        m &= m - 1u; v >>= 1;
    }
    return out;
}

extern __shared__ __attribute__((aligned(16))) unsigned char qvw_lds[];

// One pass: workgroup (tile, circuit).  LDS: the tile (16 B << T) and two tables of the local -> global index map (the low seven
// local bits, the rest), 768 B.  Every global index is tile bits on ~M plus local bits on M, both below 2^n by construction.
__global__ void __launch_bounds__(1024)
qvw_pass_kernel(int n, int T, int L, int pass, long long item0, const uint8_t* __restrict__ pairs, const double* __restrict__ gates,
                const int32_t* __restrict__ npass, const int32_t* __restrict__ first, const uint32_t* __restrict__ mask,
                cplx* __restrict__ state) {
    const long long item = item0 + blockIdx.y;
    if (pass >= npass[item]) return;                                     // workgroup-uniform: a shorter (or poisoned) circuit
    cplx* S = reinterpret_cast<cplx*>(qvw_lds);
    unsigned* tab_lo = reinterpret_cast<unsigned*>(qvw_lds + (sizeof(cplx) << T));
    unsigned* tab_hi = tab_lo + 128;
    const int tid = (int)threadIdx.x, nth = (int)blockDim.x, NT = 1 << T;
    const unsigned M = (unsigned)uniform((int)mask[(size_t)item * L + pass]);
    const int g0 = uniform(first[(size_t)item * (L + 1) + pass]), g1 = uniform(first[(size_t)item * (L + 1) + pass + 1]);
    for (int e = tid; e < 128 + (1 << (T - 7)); e += nth)
        tab_lo[e] = e < 128 ? qvw_deposit((unsigned)e, M, 0) : qvw_deposit((unsigned)(e - 128), M, 7);
    const unsigned tile = qvw_deposit((unsigned)blockIdx.x, ~M & ((1u << n) - 1u), 0);
    cplx* st = state + ((size_t)blockIdx.y << n);
    __syncthreads();
    if (pass == 0) {
        for (int j = tid; j < NT; j += nth) S[qv_slot(j)] = cplx{(tile == 0u && j == 0) ? 1.0 : 0.0, 0.0};
    } else {
        for (int j = tid; j < NT; j += nth) S[qv_slot(j)] = st[tile | tab_lo[j & 127] | tab_hi[j >> 7]];
    }
    __syncthreads();
    for (int l = g0; l < g1; ++l) {
        const uint8_t* pr = pairs + ((size_t)item * L + l) * 2;
        const int p0 = n - 1 - uniform((int)pr[0]), p1 = n - 1 - uniform((int)pr[1]);   // qubit 0 = most significant bit; both in M (the plan)
        const int l0 = __popc(M & ((1u << p0) - 1u)), l1 = __popc(M & ((1u << p1) - 1u));
        qv_apply_gate(S, NT >> 2, l0, l1, gates + ((size_t)item * L + l) * 32, tid, nth);
        __syncthreads();
    }
    for (int j = tid; j < NT; j += nth) st[tile | tab_lo[j & 127] | tab_hi[j >> 7]] = S[qv_slot(j)];
}

// Per-circuit state of the steps after the last pass (zeroed before the chunk; smallest values are kept as the largest complement).
struct QvwSel {
    unsigned long long not_mn, mx, not_above, prefix, pmask;
    unsigned hist[256];
    unsigned k, cnt_le, bad, hcount;
    int hi, pad_;
};

// amplitudes -> probabilities; smallest / largest pattern; the non-finite flag
__global__ void __launch_bounds__(256)
qvw_prob_kernel(int n, long long item0, const int32_t* __restrict__ npass, const cplx* __restrict__ state, double* __restrict__ probs,
                QvwSel* __restrict__ sel) {
    __shared__ unsigned long long s_not_mn, s_mx;
    __shared__ unsigned s_bad;
    const int c = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int np = npass[item0 + c];
    if (tid == 0) { s_not_mn = 0ull; s_mx = 0ull; s_bad = np < 0 ? 1u : 0u; }
    __syncthreads();
    const size_t base = ((size_t)c << n) + (size_t)blockIdx.x * QVW_BLOCK;
    unsigned long long lmn = ~0ull, lmx = 0ull;
    unsigned lbad = 0;
#pragma unroll 4
    for (int it = 0; it < QVW_BLOCK / 256; ++it) {
        const size_t i = base + it * 256 + tid;
        const cplx a = np > 0 ? state[i] : cplx{(blockIdx.x == 0 && it == 0 && tid == 0) ? 1.0 : 0.0, 0.0};   // no pass: |0...0>
        const double p = a.re * a.re + a.im * a.im;
        probs[i] = p;
        const unsigned long long x = (unsigned long long)__double_as_longlong(p);
        if ((x & 0x7FF0000000000000ull) == 0x7FF0000000000000ull) lbad = 1;
        lmn = x < lmn ? x : lmn; lmx = x > lmx ? x : lmx;
    }
    atomicMax(&s_not_mn, ~lmn); atomicMax(&s_mx, lmx);
    if (lbad) atomicOr(&s_bad, 1u);
    __syncthreads();
    if (tid == 0) {
        atomicMax(&sel[c].not_mn, s_not_mn); atomicMax(&sel[c].mx, s_mx);
        if (s_bad) atomicOr(&sel[c].bad, 1u);
    }
}

// one lane per circuit: where the radix select starts
__global__ void __launch_bounds__(64)
qvw_select_start_kernel(int n, int chunk, QvwSel* __restrict__ sel) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= chunk) return;
    QvwSel& s = sel[c];
    const unsigned long long mn = ~s.not_mn, diff = mn ^ s.mx;
    s.k = (1u << (n - 1)) - 1u;                                          // rank N/2 - 1
    if (s.bad || diff == 0) { s.prefix = mn; s.pmask = ~0ull; s.hi = -1; return; }
    const int hi = 63 - __clzll((long long)diff);                        // the highest bit in which two values differ
    s.pmask = ~((2ull << hi) - 1ull);
    s.prefix = mn & s.pmask;
    s.hi = hi;
}

__global__ void __launch_bounds__(256)
qvw_hist_kernel(int n, const double* __restrict__ probs, QvwSel* __restrict__ sel) {
    __shared__ unsigned hist[256];
    const int c = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int hi = sel[c].hi;
    if (hi < 0) return;                                                  // workgroup-uniform: selected already (or poisoned)
    const unsigned long long pmask = sel[c].pmask, prefix = sel[c].prefix;
    const int shift = hi >= 7 ? hi - 7 : 0;
    const unsigned dmask = (1u << (hi - shift + 1)) - 1u;
    hist[tid] = 0;
    __syncthreads();
    const size_t base = ((size_t)c << n) + (size_t)blockIdx.x * QVW_BLOCK;
#pragma unroll 4
    for (int it = 0; it < QVW_BLOCK / 256; ++it) {
        const unsigned long long x = (unsigned long long)__double_as_longlong(probs[base + it * 256 + tid]);
        if ((x & pmask) == prefix) atomicAdd(&hist[(unsigned)(x >> shift) & dmask], 1u);
    }
    __syncthreads();
    if (hist[tid]) atomicAdd(&sel[c].hist[tid], hist[tid]);
}

// one wavefront per circuit: the digit that holds rank k, four bins per lane; the histogram is left zeroed for the next round
__global__ void __launch_bounds__(64)
qvw_pick_kernel(QvwSel* __restrict__ sel) {
    QvwSel& s = sel[blockIdx.x];
    const int hi = s.hi, lane = (int)threadIdx.x;
    if (hi < 0) return;
    const int shift = hi >= 7 ? hi - 7 : 0;
    const unsigned dmask = (1u << (hi - shift + 1)) - 1u;
    const unsigned k = s.k;
    const unsigned c0 = s.hist[4 * lane], c1 = s.hist[4 * lane + 1], c2 = s.hist[4 * lane + 2], c3 = s.hist[4 * lane + 3];
    s.hist[4 * lane] = 0; s.hist[4 * lane + 1] = 0; s.hist[4 * lane + 2] = 0; s.hist[4 * lane + 3] = 0;
    const unsigned sum = c0 + c1 + c2 + c3;
    const unsigned incl = wave_scan_u32(sum, lane), excl = incl - sum;
    if (excl <= k && k < incl) {                                         // exactly one lane
        unsigned r = k - excl, d = 4 * lane;
        if (r >= c0) { r -= c0; ++d; if (r >= c1) { r -= c1; ++d; if (r >= c2) { r -= c2; ++d; } } }
        s.prefix |= (unsigned long long)d << shift;
        s.pmask |= (unsigned long long)dmask << shift;
        s.k = r;
        s.hi = shift - 1;
    }
}

// rank N/2: how many values are <= v1, and the smallest one above it
__global__ void __launch_bounds__(256)
qvw_count_kernel(int n, const double* __restrict__ probs, QvwSel* __restrict__ sel) {
    __shared__ unsigned s_cnt;
    __shared__ unsigned long long s_not_above;
    const int c = (int)blockIdx.y, tid = (int)threadIdx.x;
    if (sel[c].bad) return;
    const unsigned long long v1 = sel[c].prefix;
    if (tid == 0) { s_cnt = 0; s_not_above = 0ull; }
    __syncthreads();
    const size_t base = ((size_t)c << n) + (size_t)blockIdx.x * QVW_BLOCK;
    unsigned cnt = 0;
    unsigned long long ab = ~0ull;
#pragma unroll 4
    for (int it = 0; it < QVW_BLOCK / 256; ++it) {
        const unsigned long long x = (unsigned long long)__double_as_longlong(probs[base + it * 256 + tid]);
        if (x <= v1) ++cnt; else ab = x < ab ? x : ab;
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    if (ab != ~0ull) atomicMax(&s_not_above, ~ab);
    __syncthreads();
    if (tid == 0) {
        if (s_cnt) atomicAdd(&sel[c].cnt_le, s_cnt);
        if (s_not_above) atomicMax(&sel[c].not_above, s_not_above);
    }
}

__device__ __forceinline__ double qvw_median(const QvwSel& s, int n) {
    const unsigned long long v1 = s.prefix, v2 = s.cnt_le > (1u << (n - 1)) ? v1 : ~s.not_above;
    return 0.5 * (__longlong_as_double((long long)v1) + __longlong_as_double((long long)v2));
}

// heavy outputs: strictly above the median; mask word w holds outputs 64 w .. 64 w + 63.  part[c][block] = the heavy probability
// of the block's QVW_BLOCK outputs in one fixed order (a lane's 16 outputs in order, wave_sum, the four wavefronts in order).
__global__ void __launch_bounds__(256)
qvw_mask_kernel(int n, long long item0, double* __restrict__ probs, int write_nan, QvwSel* __restrict__ sel,
                unsigned long long* __restrict__ mask_out, double* __restrict__ part) {
    __shared__ double red[4];
    const int c = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63;
    const size_t base = ((size_t)c << n) + (size_t)blockIdx.x * QVW_BLOCK;
    const size_t W = (size_t)1 << (n - 6);
    unsigned long long* mrow = mask_out ? mask_out + (size_t)(item0 + c) * W + (size_t)blockIdx.x * (QVW_BLOCK / 64) : nullptr;
    if (sel[c].bad) {                                // a poisoned item: NaN probabilities, an empty heavy set
        if (write_nan)
            for (int it = 0; it < QVW_BLOCK / 256; ++it) probs[base + it * 256 + tid] = __builtin_nan("");
        if (mrow && tid < QVW_BLOCK / 64) mrow[tid] = 0ull;
        return;
    }
    const double median = qvw_median(sel[c], n);
    double hp = 0.0;
    unsigned hc = 0;
#pragma unroll 4
    for (int it = 0; it < QVW_BLOCK / 256; ++it) {
        const double p = probs[base + it * 256 + tid];
        const bool heavy = p > median;
        const unsigned long long word = __ballot(heavy);
        if (heavy) hp += p;
        hc += (unsigned)__popcll(word);
        if (mrow && lane == 0) mrow[(it * 256 + tid) >> 6] = word;
    }
    if (lane == 0 && hc) atomicAdd(&sel[c].hcount, hc);
    hp = wave_sum(hp);
    if (lane == 0) red[tid >> 6] = hp;
    __syncthreads();
    if (tid == 0) part[(size_t)c * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup per circuit: the blocks' heavy probabilities in order (thread t adds blocks t, t + 256, ..., then block_sum), and
// the scalar results
__global__ void __launch_bounds__(256)
qvw_finish_kernel(int n, long long item0, int nblk, const QvwSel* __restrict__ sel, const double* __restrict__ part,
                  double* __restrict__ median_out, double* __restrict__ hprob_out, int* __restrict__ hcount_out) {
    __shared__ double red[4];
    const int c = (int)blockIdx.x, tid = (int)threadIdx.x;
    double s = 0.0;
    const bool bad = sel[c].bad != 0;
    if (!bad)
        for (int j = tid; j < nblk; j += 256) s += part[(size_t)c * nblk + j];
    s = block_sum<256>(s, red);
    if (tid == 0) {
        const long long item = item0 + c;
        if (median_out) median_out[item] = bad ? __builtin_nan("") : qvw_median(sel[c], n);
        if (hprob_out) hprob_out[item] = bad ? __builtin_nan("") : s;
        if (hcount_out) hcount_out[item] = bad ? 0 : (int)sel[c].hcount;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// heavy-hitter counts: shot row -> integer (first column most significant) -> one bit of the circuit's mask, read from cache or
// HBM.  Only bit 0 of every byte is read.  Workgroup (slice, circuit) counts the shots slice, slice + gridDim.x, ... of 256.
__global__ void __launch_bounds__(256)
qvw_count_heavy_kernel(int n, long long n_shots, const uint8_t* __restrict__ bits, const unsigned long long* __restrict__ mask,
                       unsigned long long* __restrict__ counts) {
    __shared__ double red[4];
    const long long b = blockIdx.y;
    const uint8_t* rec = bits + (size_t)b * n_shots * n;
    const unsigned long long* m = mask + ((size_t)b << (n - 6));
    unsigned cnt = 0;
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < n_shots; s += (long long)gridDim.x * 256) {
        unsigned idx = 0;
        for (int q = 0; q < n; ++q) idx = (idx << 1) | (unsigned)(rec[s * n + q] & 1);
        cnt += (unsigned)((m[idx >> 6] >> (idx & 63)) & 1ull);
    }
    const double total = block_sum<256>((double)cnt, red);               // exact: a workgroup's count stays far below 2^53
    if (threadIdx.x == 0 && total > 0.0) atomicAdd(&counts[b], (unsigned long long)total);
}

static int qvw_check_width(int n_qubits, const char* who) {
    if (n_qubits < QVW_MIN_WIDTH || n_qubits > QVW_MAX_WIDTH) {
        set_error(std::string(who) + ": n_qubits must be 14..26 (narrower circuits go to the functions without _wide; got " +
                  std::to_string(n_qubits) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    return FBX_OK;
}

static int qvw_check_tile(int tile_bits, const char* who) {
    if (tile_bits != 0 && (tile_bits < QVW_MIN_TILE || tile_bits > QVW_MAX_TILE)) {
        set_error(std::string(who) + ": tile_bits must be 0 (the default) or 8..13");
        return FBX_ERR_BAD_ARG;
    }
    return FBX_OK;
}

static int qvw_check_pairs(int n_qubits, size_t n_gates, const uint8_t* pairs, const char* who) {
    for (size_t g = 0; g < n_gates; ++g)
        if (!(pairs[2 * g] < n_qubits && pairs[2 * g + 1] < n_qubits && pairs[2 * g] != pairs[2 * g + 1])) {
            set_error(std::string(who) + ": a gate needs two different qubits below n_qubits");
            return FBX_ERR_BAD_ARG;
        }
    return FBX_OK;
}

static int qvw_heavy_outputs_check(int n_qubits, int64_t B, int L, const void* pairs, const void* gates, int tile_bits, const void* probs,
                                   const void* median, const void* mask, const void* heavy_prob, const void* heavy_count) {
    FBX_REQUIRE(B >= 0 && L >= 0, "fbx_qv_heavy_outputs_wide: need B >= 0 and L >= 0");
    FBX_REQUIRE(B == 0 || L == 0 || (pairs && gates), "fbx_qv_heavy_outputs_wide: NULL pairs / gates");
    FBX_REQUIRE(probs || median || mask || heavy_prob || heavy_count, "fbx_qv_heavy_outputs_wide: no output asked for");
    FBX_TRY(qvw_check_width(n_qubits, "fbx_qv_heavy_outputs_wide"));
    return qvw_check_tile(tile_bits, "fbx_qv_heavy_outputs_wide");
}

static int qvw_launch_plan(int n, int64_t B, int L, int T, const uint8_t* d_pairs, int32_t* d_npass, int32_t* d_first, uint32_t* d_mask) {
    hipLaunchKernelGGL(qvw_plan_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream(), n, (long long)B, L, T, d_pairs,
                       d_npass, d_first, d_mask);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

// The whole computation on device pointers; `passes` launches per chunk (a bound on, or the maximum of, the circuits' pass counts).
static int qvw_run(int n, int64_t B, int L, int T, int passes, const uint8_t* d_pairs, const double* d_gates, double* d_probs_out,
                   double* d_median_out, uint64_t* d_mask_out, double* d_hprob_out, int32_t* d_hcount_out) {
    const size_t N = (size_t)1 << n, nblk = N / QVW_BLOCK;
    DevBuf plan;                                                          // [B] pass counts, [B][L + 1] first gates, [B][L] masks
    FBX_TRY(plan.alloc(sizeof(int32_t) * (size_t)B * (2 * (size_t)L + 2)));
    int32_t* d_npass = plan.as<int32_t>();
    int32_t* d_first = d_npass + B;
    uint32_t* d_lmask = reinterpret_cast<uint32_t*>(d_first + (size_t)B * (L + 1));
    FBX_TRY(qvw_launch_plan(n, B, L, T, d_pairs, d_npass, d_first, d_lmask));
    // the chunk: as many circuits as the workspace cap admits, at least one
    const size_t sel_bytes = (sizeof(QvwSel) + 15) & ~(size_t)15;
    const size_t per = 16 * N + (d_probs_out ? 0 : 8 * N) + 8 * nblk + sel_bytes;
    const double cap = option_qv_wide_workspace_mib() * 1048576.0;
    int64_t chunk = (int64_t)(cap / (double)per);
    chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(chunk, B), QVW_MAX_CHUNK));
    void* ws = nullptr;
    FBX_TRY(workspace(WS_QV_WIDE, per * (size_t)chunk, &ws));
    unsigned char* w = static_cast<unsigned char*>(ws);
    cplx* state = reinterpret_cast<cplx*>(w);                             w += 16 * N * (size_t)chunk;
    double* ws_probs = reinterpret_cast<double*>(w);                      w += (d_probs_out ? 0 : 8 * N) * (size_t)chunk;
    double* part = reinterpret_cast<double*>(w);                          w += 8 * nblk * (size_t)chunk;
    QvwSel* sel = reinterpret_cast<QvwSel*>(w);
    const size_t lds = (sizeof(cplx) << T) + 768;
    const unsigned threads = (unsigned)std::min(1024, 1 << (T - 2));
    for (int64_t item0 = 0; item0 < B; item0 += chunk) {
        const unsigned cb = (unsigned)std::min<int64_t>(chunk, B - item0);
        double* probs = d_probs_out ? d_probs_out + (size_t)item0 * N : ws_probs;
        FBX_HIP(hipMemsetAsync(sel, 0, sizeof(QvwSel) * cb, stream()));
        for (int p = 0; p < passes; ++p)
            FBX_TRY(launch_lds(qvw_pass_kernel, dim3((unsigned)(N >> T), cb), dim3(threads), lds, n, T, L, p, (long long)item0, d_pairs,
                               d_gates, d_npass, d_first, d_lmask, state));
        const dim3 grid((unsigned)nblk, cb);
        hipLaunchKernelGGL(qvw_prob_kernel, grid, dim3(256), 0, stream(), n, (long long)item0, d_npass, state, probs, sel);
        hipLaunchKernelGGL(qvw_select_start_kernel, dim3((cb + 63) / 64), dim3(64), 0, stream(), n, (int)cb, sel);
        for (int round = 0; round < 8; ++round) {
            hipLaunchKernelGGL(qvw_hist_kernel, grid, dim3(256), 0, stream(), n, probs, sel);
            hipLaunchKernelGGL(qvw_pick_kernel, dim3(cb), dim3(64), 0, stream(), sel);
        }
        hipLaunchKernelGGL(qvw_count_kernel, grid, dim3(256), 0, stream(), n, probs, sel);
        hipLaunchKernelGGL(qvw_mask_kernel, grid, dim3(256), 0, stream(), n, (long long)item0, probs, d_probs_out ? 1 : 0, sel,
                           (unsigned long long*)d_mask_out, part);
        hipLaunchKernelGGL(qvw_finish_kernel, dim3(cb), dim3(256), 0, stream(), n, (long long)item0, (int)nblk, sel, part, d_median_out,
                           d_hprob_out, d_hcount_out);
        FBX_HIP(hipGetLastError());
    }
    return FBX_OK;
}

static int qvw_count_heavy_check(int n_qubits, int64_t B, int64_t n_shots, const void* bits, const void* mask, const void* counts) {
    FBX_REQUIRE(B >= 0 && n_shots >= 0, "fbx_qv_count_heavy_wide: need B >= 0 and n_shots >= 0");
    FBX_REQUIRE(B == 0 || (mask && counts && (bits || n_shots == 0)), "fbx_qv_count_heavy_wide: NULL buffer");
    return qvw_check_width(n_qubits, "fbx_qv_count_heavy_wide");
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_qv_heavy_outputs_wide_dev(int n_qubits, int64_t B, int L, const uint8_t* d_pairs, const double* d_gates, int tile_bits,
                                  double* d_probs_out, double* d_median_out, uint64_t* d_heavy_mask_out, double* d_heavy_prob_out,
                                  int32_t* d_heavy_count_out) {
    FBX_TRY(qvw_heavy_outputs_check(n_qubits, B, L, d_pairs, d_gates, tile_bits, d_probs_out, d_median_out, d_heavy_mask_out,
                                    d_heavy_prob_out, d_heavy_count_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const int T = tile_bits ? tile_bits : QVW_DEFAULT_TILE;
    return qvw_run(n_qubits, B, L, T, qvw_pass_bound(L, T), d_pairs, d_gates, d_probs_out, d_median_out, d_heavy_mask_out,
                   d_heavy_prob_out, d_heavy_count_out);
}

int fbx_qv_heavy_outputs_wide(int n_qubits, int64_t B, int L, const uint8_t* pairs, const double* gates, int tile_bits,
                              double* probs_out, double* median_out, uint64_t* heavy_mask_out, double* heavy_prob_out,
                              int32_t* heavy_count_out) {
    FBX_TRY(qvw_heavy_outputs_check(n_qubits, B, L, pairs, gates, tile_bits, probs_out, median_out, heavy_mask_out, heavy_prob_out,
                                    heavy_count_out));
    const size_t n_gates = (size_t)B * (size_t)L;
    FBX_TRY(qvw_check_pairs(n_qubits, n_gates, pairs, "fbx_qv_heavy_outputs_wide"));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const int T = tile_bits ? tile_bits : QVW_DEFAULT_TILE;
    int passes = 0;                                   // the pairs are here: launch exactly as many passes as the longest plan has
    {
        std::vector<int32_t> first((size_t)L + 1);
        std::vector<uint32_t> lmask((size_t)L + 1);
        for (int64_t b = 0; b < B; ++b)
            passes = std::max(passes, qvw_plan_circuit(n_qubits, L, T, pairs + (size_t)b * L * 2, first.data(), lmask.data()));
    }
    const size_t n = (size_t)B, N = (size_t)1 << n_qubits, W = N / 64;
    HostIO io; uint8_t* dp; double *dg, *dprob, *dmed, *dhp; uint64_t* dmask; int32_t* dhc;
    FBX_TRY(io.in(pairs, 2 * n_gates, &dp)); FBX_TRY(io.in(gates, 32 * n_gates, &dg));
    FBX_TRY(io.out_opt(probs_out, n * N, &dprob)); FBX_TRY(io.out_opt(median_out, n, &dmed));
    FBX_TRY(io.out_opt(heavy_mask_out, n * W, &dmask)); FBX_TRY(io.out_opt(heavy_prob_out, n, &dhp));
    FBX_TRY(io.out_opt(heavy_count_out, n, &dhc));
    FBX_TRY(qvw_run(n_qubits, B, L, T, passes, dp, dg, dprob, dmed, dmask, dhp, dhc));
    return io.finish();
}

int fbx_qv_wide_plan(int n_qubits, int64_t B, int L, const uint8_t* pairs, int tile_bits, int32_t* n_passes_out,
                     int32_t* pass_first_gate_out, uint32_t* pass_local_mask_out) {
    FBX_REQUIRE(B >= 0 && L >= 0, "fbx_qv_wide_plan: need B >= 0 and L >= 0");
    FBX_REQUIRE(B == 0 || ((pairs || L == 0) && n_passes_out && pass_first_gate_out && (pass_local_mask_out || L == 0)),
                "fbx_qv_wide_plan: NULL buffer");
    FBX_TRY(qvw_check_width(n_qubits, "fbx_qv_wide_plan"));
    FBX_TRY(qvw_check_tile(tile_bits, "fbx_qv_wide_plan"));
    const size_t n_gates = (size_t)B * (size_t)L;
    FBX_TRY(qvw_check_pairs(n_qubits, n_gates, pairs, "fbx_qv_wide_plan"));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    HostIO io; uint8_t* dp; int32_t *dn, *df; uint32_t* dm;
    FBX_TRY(io.in(pairs, 2 * n_gates, &dp));
    FBX_TRY(io.out(n_passes_out, (size_t)B, &dn)); FBX_TRY(io.out(pass_first_gate_out, (size_t)B * (L + 1), &df));
    FBX_TRY(io.out(pass_local_mask_out, n_gates, &dm));
    FBX_TRY(qvw_launch_plan(n_qubits, B, L, tile_bits ? tile_bits : QVW_DEFAULT_TILE, dp, dn, df, dm));
    return io.finish();
}

int fbx_qv_count_heavy_wide_dev(int n_qubits, int64_t B, int64_t n_shots, const uint8_t* d_bits, const uint64_t* d_heavy_mask,
                                int64_t* d_counts_out) {
    FBX_TRY(qvw_count_heavy_check(n_qubits, B, n_shots, d_bits, d_heavy_mask, d_counts_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    FBX_HIP(hipMemsetAsync(d_counts_out, 0, sizeof(int64_t) * (size_t)B, stream()));
    if (n_shots == 0) return FBX_OK;
    const int64_t slices = std::min<int64_t>(64, (n_shots + 4095) / 4096);
    for (int64_t b0 = 0; b0 < B; b0 += QVW_MAX_CHUNK) {
        const unsigned cb = (unsigned)std::min<int64_t>(QVW_MAX_CHUNK, B - b0);
        hipLaunchKernelGGL(qvw_count_heavy_kernel, dim3((unsigned)slices, cb), dim3(256), 0, stream(), n_qubits, (long long)n_shots,
                           d_bits + (size_t)b0 * n_shots * n_qubits,
                           (const unsigned long long*)d_heavy_mask + ((size_t)b0 << (n_qubits - 6)),
                           (unsigned long long*)d_counts_out + b0);
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_qv_count_heavy_wide(int n_qubits, int64_t B, int64_t n_shots, const uint8_t* bits, const uint64_t* heavy_mask,
                            int64_t* counts_out) {
    FBX_TRY(qvw_count_heavy_check(n_qubits, B, n_shots, bits, heavy_mask, counts_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t W = (size_t)1 << (n_qubits - 6);
    HostIO io; uint8_t* db; uint64_t* dm; int64_t* dc;
    FBX_TRY(io.in(bits, (size_t)B * n_shots * n_qubits, &db)); FBX_TRY(io.in(heavy_mask, (size_t)B * W, &dm));
    FBX_TRY(io.out(counts_out, (size_t)B, &dc));
    FBX_TRY(fbx_qv_count_heavy_wide_dev(n_qubits, B, n_shots, db, dm, dc));
    return io.finish();
}

}  // C ABI
