// fbx_histogram.hip -- histograms of measured bitstrings, batched: readout confusion matrices (readout.py:69-180, 236-335), the
// ripple-carry adder's success probabilities and error-weight distributions (classical_logic/ripple_carry_adder.py:317-384) and
// the GHZ statistics (entangled_states.py:36-51) are all "how often did each bitstring / each Hamming weight occur in a record".
//
// bit_histogram_kernel: a byte-stream reduction shaped like fbx_shots.hip and qv_count_record (fbx_qvolume.hip): one WAVEFRONT
// per short record (four records per 256-thread workgroup, no workgroup barrier), one workgroup per long record, a grid-stride
// loop over the records.  A record of 1..8 columns is read in runs of 16 shots = n_cols 16-byte vectors per lane from the first
// shot that starts on a 16-byte boundary; the shots around the runs, and records of more than 8 columns, go byte-wise.
//
// LDS, per wavefront (HistWave, 4736 B; 18.5 KB per workgroup): a private histogram of up to 1024 32-bit counters, the record's
// column selection and expected pattern, and -- for the vector path -- a 256-entry table from the 8 low bits of a shot (bit q =
// column q) to its bin, built once per record from the selection, the pattern and the kind.  A shot then costs one LDS read and
// one integer LDS add (ds_add_u32); the counters are private to the wavefront, so a record where every shot falls into ONE bin
// serialises inside one instruction only.  In the workgroup form the four private histograms are summed after a barrier.  One
// wavefront or one workgroup owns a record: no global atomics, the bins leave as plain vector stores, and since the counts are
// integers the result does not depend on the launch shape.
//
// marginalize_confusion_kernel: readout.py:183-233 for a batch of 2^n x 2^n matrices -- every output element is the sum of the
// 4^(n-k) inputs that agree with it on the kept bits, in ONE order (a thread per element and ascending traced index while the sum
// is short, a wavefront per element with lane-strided partial sums and the fixed wave_sum tree from 64 terms on), over 2^(n-k).
#include "fbx_common.hpp"

namespace fbx {

constexpr int FBX_HIST_MAX_JOINT_K = 10;
constexpr long long FBX_HIST_MAX_SHOTS = 2147483647ll;       // 32-bit counters in LDS

struct HistWave {
    unsigned hist[1 << FBX_HIST_MAX_JOINT_K];
    unsigned short lut[256];
    unsigned char sel[64], ex[64];
};

// bin of a shot whose column q holds bit q of `shot` (JOINT: first selected column most significant; WEIGHT: Hamming weight)
__device__ __forceinline__ unsigned hist_bin_of(const HistWave& w, unsigned long long shot, int k, int kind) {
    unsigned idx = 0;
    for (int i = 0; i < k; ++i) {
        const unsigned bit = (unsigned)((shot >> w.sel[i]) & 1ull) ^ w.ex[i];
        idx = kind == FBX_HIST_JOINT ? (idx << 1) | bit : idx + bit;
    }
    return idx;
}

template <int NC>      // NC = 1..8 columns: 16-byte vector path with the table
__device__ __forceinline__ void hist_record_vec(const uint8_t* __restrict__ bits, long long n_shots, HistWave& w, int tid, int nth) {
    long long head = n_shots, runs = 0;
    for (int s = 0; s < 16; ++s)
        if ((((uintptr_t)bits + (uintptr_t)(s * NC)) & 15) == 0) { head = s; break; }
    if (head < n_shots) {
        runs = (n_shots - head) / 16;
        const ulonglong2* v = reinterpret_cast<const ulonglong2*>(bits + head * NC);
        for (long long r = tid; r < runs; r += nth) {
            unsigned long long x[2 * NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) { const ulonglong2 t = v[r * NC + c]; x[2 * c] = t.x; x[2 * c + 1] = t.y; }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                unsigned m = 0;
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    const int byte = j * NC + q;
                    m |= (unsigned)((x[byte >> 3] >> (8 * (byte & 7))) & 1ull) << q;
                }
                atomicAdd(&w.hist[w.lut[m]], 1u);
            }
        }
    } else head = n_shots;
    const long long tail0 = head + runs * 16, rest = head + (n_shots - tail0);
    for (long long i = tid; i < rest; i += nth) {
        const long long s = i < head ? i : tail0 + (i - head);
        unsigned m = 0;
#pragma unroll
        for (int q = 0; q < NC; ++q) m |= (unsigned)(bits[s * NC + q] & 1) << q;
        atomicAdd(&w.hist[w.lut[m]], 1u);
    }
}

// any column count: byte-wise, the bin straight from the selected bytes
__device__ __forceinline__ void hist_record_generic(const uint8_t* __restrict__ bits, long long n_shots, int n_cols, int k, int kind,
                                                    HistWave& w, int tid, int nth) {
    for (long long s = tid; s < n_shots; s += nth) {
        const uint8_t* row = bits + s * n_cols;
        unsigned idx = 0;
        for (int i = 0; i < k; ++i) {
            const unsigned bit = (unsigned)(row[w.sel[i]] & 1) ^ w.ex[i];
            idx = kind == FBX_HIST_JOINT ? (idx << 1) | bit : idx + bit;
        }
        atomicAdd(&w.hist[idx], 1u);
    }
}

template <int NC, bool PER_WAVE>      // NC = 0: any n_cols, byte-wise
__global__ void __launch_bounds__(256)
bit_histogram_kernel(int n_cols, long long B, long long n_shots, const uint8_t* __restrict__ bits, int k,
                     const uint8_t* __restrict__ cols, int cols_shared, const uint8_t* __restrict__ expected, int kind,
                     long long* __restrict__ counts_out) {
    __shared__ HistWave hw[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    HistWave& my = hw[wave];
    const int bins = kind == FBX_HIST_JOINT ? 1 << k : k + 1;
    const int tid = PER_WAVE ? lane : (int)threadIdx.x, nth = PER_WAVE ? 64 : 256;
    const long long first = PER_WAVE ? (long long)blockIdx.x * 4 + wave : blockIdx.x;
    const long long stride = PER_WAVE ? (long long)gridDim.x * 4 : gridDim.x;
    for (long long b = first; b < B; b += stride) {
        // every wavefront keeps its own copy of the record's tables and clears its own bins: nothing to wait for but itself
        int c = 0, e = 0;
        if (lane < k) {
            c = cols ? cols[(cols_shared ? 0 : b * k) + lane] : lane;
            e = expected ? expected[b * k + lane] & 1 : 0;
        }
        const bool bad = __ballot(c >= n_cols) != 0ull;       // wave-uniform; only the _dev form can meet it: never index outside a shot
        my.sel[lane] = (unsigned char)c; my.ex[lane] = (unsigned char)e;
        for (int i = lane; i < bins; i += 64) my.hist[i] = 0;
        FBX_WAVE_SYNC();
        if (!bad) {
            const uint8_t* rec = bits + b * n_shots * n_cols;
            if constexpr (NC > 0) {
                for (int m = lane; m < (1 << NC); m += 64) my.lut[m] = (unsigned short)hist_bin_of(my, (unsigned long long)m, k, kind);
                FBX_WAVE_SYNC();
                hist_record_vec<NC>(rec, n_shots, my, tid, nth);
            } else {
                hist_record_generic(rec, n_shots, n_cols, k, kind, my, tid, nth);
            }
        }
        long long* out = counts_out + b * bins;
        if constexpr (PER_WAVE) {
            FBX_WAVE_SYNC();
            for (int i = lane; i < bins; i += 64) out[i] = bad ? -1ll : (long long)my.hist[i];
            FBX_WAVE_SYNC();                                    // the bins are cleared again for the wavefront's next record
        } else {
            __syncthreads();
            for (int i = threadIdx.x; i < bins; i += 256)
                out[i] = bad ? -1ll : ((long long)hw[0].hist[i] + (long long)hw[1].hist[i]) + ((long long)hw[2].hist[i] + (long long)hw[3].hist[i]);
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256)
counts_to_frequencies_kernel(long long n, const long long* __restrict__ counts, double denom, double* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = (double)counts[i] / denom;
}

// bit j of v goes to the j-th lowest set bit of mask
__device__ __forceinline__ unsigned deposit_bits(unsigned v, unsigned mask) {
    unsigned r = 0;
    for (; mask; mask &= mask - 1, v >>= 1)
        if (v & 1u) r |= mask & (0u - mask);
    return r;
}

// a thread per output element: 4^(n-k) <= 16 terms, traced row index ascending, traced column index ascending inside
__global__ void __launch_bounds__(256)
marginalize_thread_kernel(int n, int k, unsigned keepmask, long long B, const double* __restrict__ in, double* __restrict__ out) {
    const long long N = 1ll << n, M = 1ll << k, total = B * M * M;
    const unsigned R = 1u << (n - k), tmask = ((unsigned)N - 1u) & ~keepmask;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long b = idx / (M * M), e = idx % (M * M);
        const unsigned br = deposit_bits((unsigned)(e / M), keepmask), bc = deposit_bits((unsigned)(e % M), keepmask);
        const double* a = in + b * N * N;
        double s = 0.0;
        for (unsigned tr = 0; tr < R; ++tr) {
            const long long row = (long long)(br | deposit_bits(tr, tmask)) * N;
            for (unsigned tc = 0; tc < R; ++tc) s += a[row + (bc | deposit_bits(tc, tmask))];
        }
        out[idx] = s / (double)R;
    }
}

// a wavefront per output element (64 terms and more): lane l sums terms l, l + 64, ... in order, then the fixed tree of wave_sum
__global__ void __launch_bounds__(256)
marginalize_wave_kernel(int n, int k, unsigned keepmask, long long B, const double* __restrict__ in, double* __restrict__ out) {
    const long long N = 1ll << n, M = 1ll << k, total = B * M * M;
    const int lane = threadIdx.x & 63, shift = n - k;
    const unsigned R = 1u << shift, T = R * R, tmask = ((unsigned)N - 1u) & ~keepmask;
    for (long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); idx < total; idx += (long long)gridDim.x * 4) {
        const long long b = idx / (M * M), e = idx % (M * M);
        const unsigned br = deposit_bits((unsigned)(e / M), keepmask), bc = deposit_bits((unsigned)(e % M), keepmask);
        const double* a = in + b * N * N;
        double s = 0.0;
        for (unsigned t = lane; t < T; t += 64)
            s += a[(long long)(br | deposit_bits(t >> shift, tmask)) * N + (bc | deposit_bits(t & (R - 1u), tmask))];
        s = wave_sum(s);
        if (lane == 0) out[idx] = s / (double)R;
    }
}

static int hist_check(int n_cols, int64_t B, int64_t n_shots, const void* bits, int k, const void* cols, int kind, const void* counts) {
    FBX_REQUIRE(n_cols >= 1 && n_cols <= 64, "fbx_bit_histogram: n_cols must be 1..64");
    FBX_REQUIRE(kind == FBX_HIST_JOINT || kind == FBX_HIST_WEIGHT, "fbx_bit_histogram: kind must be FBX_HIST_JOINT or FBX_HIST_WEIGHT");
    if (kind == FBX_HIST_JOINT) FBX_REQUIRE(k >= 1 && k <= FBX_HIST_MAX_JOINT_K, "fbx_bit_histogram: k must be 1..10 for FBX_HIST_JOINT");
    else FBX_REQUIRE(k >= 1 && k <= 64, "fbx_bit_histogram: k must be 1..64 for FBX_HIST_WEIGHT");
    FBX_REQUIRE(cols != nullptr || k <= n_cols, "fbx_bit_histogram: k exceeds n_cols and cols is NULL");
    FBX_REQUIRE(n_shots >= 1 && n_shots <= FBX_HIST_MAX_SHOTS, "fbx_bit_histogram: n_shots must be 1..2^31 - 1 (32-bit counters)");
    FBX_REQUIRE(B >= 0, "fbx_bit_histogram: B must not be negative");
    FBX_REQUIRE(B == 0 || (bits && counts), "fbx_bit_histogram: NULL bits / counts_out buffer");
    return FBX_OK;
}

static int freq_check(int64_t n, const void* counts, int64_t denom, const void* out) {
    FBX_REQUIRE(n >= 0, "fbx_counts_to_frequencies: n must not be negative");
    FBX_REQUIRE(denom >= 1, "fbx_counts_to_frequencies: denom must be positive");
    FBX_REQUIRE(n == 0 || (counts && out), "fbx_counts_to_frequencies: NULL buffer");
    return FBX_OK;
}

static int marginalize_check(int n_qubits, int64_t B, int k, const uint8_t* keep, const void* in, const void* out, unsigned* keepmask) {
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 10, "fbx_marginalize_confusion: n_qubits must be 1..10");
    FBX_REQUIRE(k >= 1 && k <= n_qubits, "fbx_marginalize_confusion: k must be 1..n_qubits");
    FBX_REQUIRE(keep != nullptr, "fbx_marginalize_confusion: NULL keep");
    unsigned mask = 0;
    for (int i = 0; i < k; ++i) {
        FBX_REQUIRE(keep[i] < n_qubits, "fbx_marginalize_confusion: a keep entry is not below n_qubits");
        FBX_REQUIRE(i == 0 || keep[i] > keep[i - 1], "fbx_marginalize_confusion: keep must be strictly ascending");
        mask |= 1u << (n_qubits - 1 - keep[i]);                 // position 0 = the most significant bit of the index
    }
    FBX_REQUIRE(B >= 0, "fbx_marginalize_confusion: B must not be negative");
    FBX_REQUIRE(B == 0 || (in && out), "fbx_marginalize_confusion: NULL in / out buffer");
    *keepmask = mask;
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_bit_histogram_dev(int n_cols, int64_t B, int64_t n_shots, const uint8_t* d_bits, int k, const uint8_t* d_cols, int cols_shared,
                          const uint8_t* d_expected, int kind, int64_t* d_counts_out) {
    FBX_TRY(hist_check(n_cols, B, n_shots, d_bits, k, d_cols, kind, d_counts_out));
    if (B == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    const bool per_wave = n_shots * n_cols < FBX_RECORD_WAVE_BYTES && B >= 4;
    const int64_t units = per_wave ? (B + 3) / 4 : B;
    const unsigned grid = (unsigned)(units < 256 * 16 ? units : 256 * 16);
#define FBX_HIST_LAUNCH(NC) do { \
        if (per_wave) hipLaunchKernelGGL((bit_histogram_kernel<NC, true>), dim3(grid), dim3(256), 0, stream(), n_cols, (long long)B, \
                                         (long long)n_shots, d_bits, k, d_cols, cols_shared, d_expected, kind, (long long*)d_counts_out); \
        else hipLaunchKernelGGL((bit_histogram_kernel<NC, false>), dim3(grid), dim3(256), 0, stream(), n_cols, (long long)B, \
                                (long long)n_shots, d_bits, k, d_cols, cols_shared, d_expected, kind, (long long*)d_counts_out); } while (0)
    switch (n_cols) {
        case 1: FBX_HIST_LAUNCH(1); break;
        case 2: FBX_HIST_LAUNCH(2); break;
        case 3: FBX_HIST_LAUNCH(3); break;
        case 4: FBX_HIST_LAUNCH(4); break;
        case 5: FBX_HIST_LAUNCH(5); break;
        case 6: FBX_HIST_LAUNCH(6); break;
        case 7: FBX_HIST_LAUNCH(7); break;
        case 8: FBX_HIST_LAUNCH(8); break;
        default: FBX_HIST_LAUNCH(0); break;
    }
#undef FBX_HIST_LAUNCH
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_bit_histogram(int n_cols, int64_t B, int64_t n_shots, const uint8_t* bits, int k, const uint8_t* cols, int cols_shared,
                      const uint8_t* expected, int kind, int64_t* counts_out) {
    FBX_TRY(hist_check(n_cols, B, n_shots, bits, k, cols, kind, counts_out));
    if (B == 0) return FBX_OK;
    const size_t n_sel = cols ? (cols_shared ? (size_t)k : (size_t)B * k) : 0;
    for (size_t i = 0; i < n_sel; ++i) FBX_REQUIRE(cols[i] < n_cols, "fbx_bit_histogram: a cols entry is not below n_cols");
    FBX_TRY(ensure_device());
    const size_t bins = kind == FBX_HIST_JOINT ? (size_t)1 << k : (size_t)k + 1;
    HostIO io; uint8_t *db, *dc = nullptr, *de = nullptr; int64_t* dout;
    FBX_TRY(io.in(bits, (size_t)B * n_shots * n_cols, &db));
    if (cols) FBX_TRY(io.in(cols, n_sel, &dc));
    if (expected) FBX_TRY(io.in(expected, (size_t)B * k, &de));
    FBX_TRY(io.out(counts_out, (size_t)B * bins, &dout));
    FBX_TRY(fbx_bit_histogram_dev(n_cols, B, n_shots, db, k, dc, cols_shared, de, kind, dout));
    return io.finish();
}

int fbx_counts_to_frequencies_dev(int64_t n, const int64_t* d_counts, int64_t denom, double* d_out) {
    FBX_TRY(freq_check(n, d_counts, denom, d_out));
    if (n == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    const long long want = ((long long)n + 255) / 256;
    hipLaunchKernelGGL(counts_to_frequencies_kernel, dim3((unsigned)(want < 256 * 32 ? want : 256 * 32)), dim3(256), 0, stream(),
                       (long long)n, (const long long*)d_counts, (double)denom, d_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_counts_to_frequencies(int64_t n, const int64_t* counts, int64_t denom, double* out) {
    FBX_TRY(freq_check(n, counts, denom, out));
    if (n == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    HostIO io; int64_t* dc; double* dout;
    FBX_TRY(io.in(counts, (size_t)n, &dc)); FBX_TRY(io.out(out, (size_t)n, &dout));
    FBX_TRY(fbx_counts_to_frequencies_dev(n, dc, denom, dout));
    return io.finish();
}

int fbx_marginalize_confusion_dev(int n_qubits, int64_t B, int k, const uint8_t* keep, const double* d_in, double* d_out) {
    unsigned keepmask = 0;
    FBX_TRY(marginalize_check(n_qubits, B, k, keep, d_in, d_out, &keepmask));
    if (B == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    const long long total = (long long)B << (2 * k);
    if (n_qubits - k <= 2) {
        const long long want = (total + 255) / 256;
        hipLaunchKernelGGL(marginalize_thread_kernel, dim3((unsigned)(want < 256 * 32 ? want : 256 * 32)), dim3(256), 0, stream(),
                           n_qubits, k, keepmask, (long long)B, d_in, d_out);
    } else {
        const long long want = (total + 3) / 4;
        hipLaunchKernelGGL(marginalize_wave_kernel, dim3((unsigned)(want < 256 * 16 ? want : 256 * 16)), dim3(256), 0, stream(),
                           n_qubits, k, keepmask, (long long)B, d_in, d_out);
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_marginalize_confusion(int n_qubits, int64_t B, int k, const uint8_t* keep, const double* in, double* out) {
    unsigned keepmask = 0;
    FBX_TRY(marginalize_check(n_qubits, B, k, keep, in, out, &keepmask));
    if (B == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    HostIO io; double *din, *dout;
    FBX_TRY(io.in(in, (size_t)B << (2 * n_qubits), &din)); FBX_TRY(io.out(out, (size_t)B << (2 * k), &dout));
    FBX_TRY(fbx_marginalize_confusion_dev(n_qubits, B, k, keep, din, dout));
    return io.finish();
}

}  // extern "C"
