// fbx_rpe.hip -- robust phase estimation (robust_phase_estimation.py:361-521), batched: the phase recursion of
// estimate_phase_from_moments one estimate per LANE (fbx_rpe_phase), the same recursion fed straight from shot bytes one estimate
// per WAVEFRONT (fbx_rpe_from_shots), and the circular mean / standard deviation of bootstrap phases (fbx_circular_stats).
//
// The recursion is discontinuous: a last-bit difference in `r < r_std` ends an item or does not, and one in the offset at the end
// of a window moves the phase by the window's width.  Every operation of the reference is therefore performed in its order, in
// fp64, without contraction into fused multiply-adds (rpe_step is compiled with contract(off)); what is left between the device
// and numpy is the last bits of atan2.
//
// fbx_rpe_from_shots: an estimate owns 2 K records (X and Y basis, K depths) of n_shots x n_qubits bytes.  Its wavefront takes
// the records depth by depth, the X and the Y record of a depth together; a lane's unit is the shortest run of whole shots that
// is a whole number of 16-byte vectors (16 / gcd(n_qubits, 16) shots = n_qubits / gcd vectors; one vector for 1, 2, 4 and 8
// qubits, so the 64 lanes of a load instruction read 1 KiB of consecutive bytes), from the first shot of the record that starts on
// a 16-byte boundary; the shots around the runs go byte-wise.  The measured column is picked with a byte pattern of period n_qubits,
// its XOR with the Z column by XOR-ing the run with itself shifted by the distance of the two columns.  Counts are integers; lane 0
// turns them into moments and advances the recursion, and once an item has ended (and no moments are asked for) the remaining
// depths of that item are not read.
#include "fbx_sim_shared.hpp"      // rpe_moment, shared with fbx_rpe_sim.hip

namespace fbx {

constexpr int RPE_MAX_DEPTHS = 62;      // depth 2^j must stay an exact double AND an int64 (the reference's k // 2)

// Python's float %, for a positive divisor: the result carries the divisor's sign
__device__ __forceinline__ double py_mod_pos(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) { if (m < 0.0) m += b; }
    else m = 0.0;
    return m;
}

struct RpeState {
    double theta = 0.0;     // theta_est
    int used = 0;           // iterations taken so far
    bool stopped = false;   // r < r_std met
    bool bad = false;       // a non-finite moment met while the item was running
};

// the moments the recursion consumes at one depth: the plain ones, or the post-selected combination of :496-504
struct RpeMoments { double x, y, xs, ys; };

__device__ __forceinline__ RpeMoments rpe_select(double x, double y, double xe, double ye, bool partner, double xz, double yz,
                                                 double xze, double yze, int errors_are_variances, int post_select) {
#pragma clang fp contract(off)
    if (errors_are_variances) { xe = sqrt(xe); ye = sqrt(ye); xze = sqrt(xze); yze = sqrt(yze); }
    RpeMoments m{x, y, xe, ye};
    if (partner) {
        m.x = post_select == 0 ? x + xz : x - xz;
        m.y = post_select == 0 ? y + yz : y - yz;
        m.xs = sqrt(xze * xze + xe * xe);
        m.ys = sqrt(yze * yze + ye * ye);
    }
    return m;
}

__device__ __forceinline__ bool rpe_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }    // false for NaN

// iteration j of :378-402 on a running item; r / angle are the bloch_data row (NaN when the item ends here)
__device__ __forceinline__ void rpe_step(RpeState& st, int j, const RpeMoments& m, double& r_out, double& angle_out) {
#pragma clang fp contract(off)
    r_out = __builtin_nan(""); angle_out = __builtin_nan("");
    if (st.stopped || st.bad) return;
    if (!(rpe_finite(m.x) && rpe_finite(m.y) && rpe_finite(m.xs) && rpe_finite(m.ys))) { st.bad = true; return; }
    const double k = (double)(1ull << j);
    const double r = sqrt(m.x * m.x + m.y * m.y);
    const double r_std = sqrt(m.xs * m.xs + m.ys * m.ys);
    if (r < r_std) { st.stopped = true; return; }
    const double theta_j = atan2(m.y, m.x) / k;
    const double plus_or_minus = 3.141592653589793 / k;
    const double low = st.theta - plus_or_minus;
    const double offset = py_mod_pos(theta_j - low, 2.0 * plus_or_minus);
    st.theta = offset + low;             // (where the offset rounds up to the window's width the reference asserts; the value is kept)
    st.used = j + 1;
    r_out = r; angle_out = st.theta * k;
}

__device__ __forceinline__ double rpe_finish(const RpeState& st) {
    return st.bad ? __builtin_nan("") : py_mod_pos(st.theta, 6.283185307179586);
}

// ------------------------------------------------------------------------------------------------ (a) one estimate per lane
__global__ void __launch_bounds__(256)
rpe_phase_kernel(long long B, int K, const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ xe,
                 const double* __restrict__ ye, const double* __restrict__ xz, const double* __restrict__ yz,
                 const double* __restrict__ xze, const double* __restrict__ yze, int errors_are_variances, int post_select,
                 double* __restrict__ phase_out, int* __restrict__ depth_out, double* __restrict__ bloch_out) {
    const bool partner = xz != nullptr;
    for (long long b = blockIdx.x * (long long)blockDim.x + threadIdx.x; b < B; b += (long long)gridDim.x * blockDim.x) {
        RpeState st;
        const long long row = b * K;
        for (int j = 0; j < K; ++j) {
            if (st.stopped || st.bad) break;
            const long long i = row + j;
            const RpeMoments m = rpe_select(x[i], y[i], xe[i], ye[i], partner, partner ? xz[i] : 0.0, partner ? yz[i] : 0.0,
                                            partner ? xze[i] : 0.0, partner ? yze[i] : 0.0, errors_are_variances, post_select);
            double r, a;
            rpe_step(st, j, m, r, a);
            if (bloch_out) { bloch_out[2 * i] = r; bloch_out[2 * i + 1] = a; }
        }
        if (bloch_out) {
            const double nan = __builtin_nan("");
            for (int j = st.bad ? 0 : st.used; j < K; ++j) { bloch_out[2 * (row + j)] = nan; bloch_out[2 * (row + j) + 1] = nan; }
        }
        if (phase_out) phase_out[b] = rpe_finish(st);
        if (depth_out) depth_out[b] = st.used;
    }
}

// ------------------------------------------------------------------------------------------------ (b) one estimate per wavefront
constexpr int rpe_gcd16(int n) { return (n % 16 == 0) ? 16 : (n % 8 == 0) ? 8 : (n % 4 == 0) ? 4 : (n % 2 == 0) ? 2 : 1; }

// One record: c1 += shots with b[col] = 1, c2 += shots with b[col] ^ b[zcol] = 1 (zcol >= 0 only), over this lane's share.
template <int NQ>
__device__ __forceinline__ void rpe_count_record(const uint8_t* __restrict__ bits, long long n_shots, int col, int zcol, int lane,
                                                 const unsigned long long* pat, long long& c1, long long& c2) {
    constexpr int G = rpe_gcd16(NQ), V = NQ / G, S = 16 / G, W = 2 * V;     // vectors, shots and 64-bit words per run
    long long head = n_shots, runs = 0;
    for (int s = 0; s < 16; ++s)
        if ((((uintptr_t)bits + (uintptr_t)(s * NQ)) & 15) == 0) { head = s; break; }
    if (head < n_shots) {
        runs = (n_shots - head) / S;
        const ulonglong2* v = reinterpret_cast<const ulonglong2*>(bits + head * NQ);
        const int d = zcol - col;                                            // wave-uniform, -7..7
        for (long long r = lane; r < runs; r += 64) {
            unsigned long long w[W + 2];                                     // w[1 + i] = word i of the run, zero on both sides
            w[0] = 0ull; w[W + 1] = 0ull;
#pragma unroll
            for (int i = 0; i < V; ++i) { const ulonglong2 t = v[r * V + i]; w[1 + 2 * i] = t.x; w[2 + 2 * i] = t.y; }
#pragma unroll
            for (int i = 0; i < W; ++i) c1 += __popcll(w[1 + i] & pat[i]);
            if (zcol >= 0) {
                // the byte at distance d of every byte: the run as one little-endian string, shifted by d bytes.  A byte that
                // comes in from outside the run only lands where the pattern is zero (both columns of a shot lie in its run).
                if (d > 0) {
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        const unsigned long long sh = (w[1 + i] >> (8 * d)) | (w[2 + i] << (64 - 8 * d));
                        c2 += __popcll((w[1 + i] ^ sh) & pat[i]);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        const unsigned long long sh = (w[1 + i] << (-8 * d)) | (w[i] >> (64 + 8 * d));
                        c2 += __popcll((w[1 + i] ^ sh) & pat[i]);
                    }
                }
            }
        }
    } else head = n_shots;
    const long long tail0 = head + runs * S, rest = head + (n_shots - tail0);
    for (long long k = lane; k < rest; k += 64) {
        const long long s = k < head ? k : tail0 + (k - head);
        const int a = bits[s * NQ + col] & 1;
        c1 += a;
        if (zcol >= 0) c2 += a ^ (bits[s * NQ + zcol] & 1);
    }
}

template <int NQ>
__global__ void __launch_bounds__(256)
rpe_shots_kernel(long long B, int K, long long n_shots, const uint8_t* __restrict__ x_bits, const uint8_t* __restrict__ y_bits,
                 int col, int zcol, int post_select, double* __restrict__ phase_out, int* __restrict__ depth_out,
                 double* __restrict__ bloch_out, double* __restrict__ moments_out) {
    constexpr int W = 2 * (NQ / rpe_gcd16(NQ));
    const int lane = threadIdx.x & 63;
    unsigned long long pat[W];                       // 0x01 at every byte of the run that belongs to column `col`
#pragma unroll
    for (int i = 0; i < W; ++i) {
        unsigned long long m = 0;
#pragma unroll
        for (int byte = 0; byte < 8; ++byte) m |= (unsigned long long)(((8 * i + byte) % NQ) == col ? 1 : 0) << (8 * byte);
        pat[i] = m;
    }
    const long long record = n_shots * NQ;
    const double nan = __builtin_nan("");
    for (long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); b < B; b += (long long)gridDim.x * 4) {
        RpeState st;
        for (int j = 0; j < K; ++j) {
            const long long i = b * K + j;
            long long cx1 = 0, cx2 = 0, cy1 = 0, cy2 = 0;
            rpe_count_record<NQ>(x_bits + i * record, n_shots, col, zcol, lane, pat, cx1, cx2);
            rpe_count_record<NQ>(y_bits + i * record, n_shots, col, zcol, lane, pat, cy1, cy2);
            const long long nx = (long long)wave_sum((double)cx1), ny = (long long)wave_sum((double)cy1);   // exact: below 2^53
            long long nxz = 0, nyz = 0;
            if (zcol >= 0) { nxz = (long long)wave_sum((double)cx2); nyz = (long long)wave_sum((double)cy2); }
            int go = 0;
            if (lane == 0) {
                double mx, vx, my, vy, mxz = 0.0, vxz = 0.0, myz = 0.0, vyz = 0.0;
                rpe_moment(nx, n_shots, mx, vx); rpe_moment(ny, n_shots, my, vy);
                if (zcol >= 0) { rpe_moment(nxz, n_shots, mxz, vxz); rpe_moment(nyz, n_shots, myz, vyz); }
                const RpeMoments m = rpe_select(mx, my, vx, vy, zcol >= 0, mxz, myz, vxz, vyz, 1, post_select);
                if (moments_out) { double* o = moments_out + 4 * i; o[0] = m.x; o[1] = m.y; o[2] = m.xs; o[3] = m.ys; }
                double r, a;
                rpe_step(st, j, m, r, a);
                if (bloch_out) { bloch_out[2 * i] = r; bloch_out[2 * i + 1] = a; }
                go = (st.stopped || st.bad) ? 0 : 1;
            }
            go = uniform(go);
            if (!go && !moments_out) break;          // the item has ended: its deeper records are not read
        }
        if (lane == 0) {
            if (bloch_out)
                for (int j = st.bad ? 0 : st.used; j < K; ++j) { bloch_out[2 * (b * K + j)] = nan; bloch_out[2 * (b * K + j) + 1] = nan; }
            if (phase_out) phase_out[b] = rpe_finish(st);
            if (depth_out) depth_out[b] = st.used;
        }
    }
}

template <int NQ>
static int launch_rpe_shots(int64_t B, int K, int64_t n_shots, const uint8_t* x_bits, const uint8_t* y_bits, int col, int zcol,
                            int post_select, double* phase, int32_t* depth, double* bloch, double* moments) {
    const int64_t units = (B + 3) / 4;
    const unsigned grid = (unsigned)(units < 256 * 16 ? units : 256 * 16);
    hipLaunchKernelGGL((rpe_shots_kernel<NQ>), dim3(grid), dim3(256), 0, stream(), (long long)B, K, (long long)n_shots, x_bits,
                       y_bits, col, zcol, post_select, phase, (int*)depth, bloch, moments);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

// ------------------------------------------------------------------------------------------------ (c) circular statistics
// One item per thread, its R angles in order (consecutive threads read consecutive doubles of a row); compensated (Neumaier)
// sums of sin and cos, so the result does not depend on R beyond the last bits and repeated calls agree bit for bit.
__global__ void __launch_bounds__(256)
circular_stats_kernel(long long R, long long B, const double* __restrict__ angles, double* __restrict__ mean_out,
                      double* __restrict__ std_out, int* __restrict__ nan_out) {
    for (long long b = blockIdx.x * (long long)blockDim.x + threadIdx.x; b < B; b += (long long)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        double ss = 0.0, sc = 0.0, cs = 0.0, cc = 0.0;      // sums and their compensations
        long long skipped = 0;
        for (long long r = 0; r < R; ++r) {
            const double a = angles[r * B + b];
            if (a != a) { ++skipped; continue; }
            double s, c;
            sincos(a, &s, &c);
            double t = ss + s;
            sc += fabs(ss) >= fabs(s) ? (ss - t) + s : (s - t) + ss;
            ss = t;
            t = cs + c;
            cc += fabs(cs) >= fabs(c) ? (cs - t) + c : (c - t) + cs;
            cs = t;
        }
        const long long n = R - skipped;
        double mean = __builtin_nan(""), sd = __builtin_nan("");
        if (n > 0) {
            const double ms = (ss + sc) / (double)n, mc = (cs + cc) / (double)n;
            mean = py_mod_pos(atan2(ms, mc), 6.283185307179586);
            const double rbar = sqrt(ms * ms + mc * mc);
            const double v = -2.0 * log(rbar);
            sd = v > 0.0 ? sqrt(v) : (v <= 0.0 ? 0.0 : v);      // rbar rounded above 1: no spread; NaN stays NaN
        }
        if (mean_out) mean_out[b] = mean;
        if (std_out) std_out[b] = sd;
        if (nan_out) nan_out[b] = (int)(skipped < 2147483647ll ? skipped : 2147483647ll);
    }
}

static int rpe_check_depths(int K, const char* who) {
    if (K > RPE_MAX_DEPTHS) {
        set_error(std::string(who) + ": at most 62 depths (depth 2^j must stay an exact integer; got " + std::to_string(K) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    return FBX_OK;
}

static int rpe_phase_check(int64_t B, int K, const void* x, const void* y, const void* x_err, const void* y_err, const void* xz,
                           const void* yz, const void* xz_err, const void* yz_err, int post_select, const void* phase,
                           const void* depth, const void* bloch) {
    FBX_REQUIRE(B >= 0 && K >= 1, "fbx_rpe_phase: need B >= 0 and K >= 1");
    FBX_REQUIRE(B == 0 || (x && y && x_err && y_err), "fbx_rpe_phase: NULL moments");
    FBX_REQUIRE((xz != nullptr) == (yz != nullptr) && (xz != nullptr) == (xz_err != nullptr) && (xz != nullptr) == (yz_err != nullptr),
                "fbx_rpe_phase: the four partner arrays come together or not at all");
    FBX_REQUIRE(post_select == 0 || post_select == 1, "fbx_rpe_phase: post_select must be 0 or 1");
    FBX_REQUIRE(phase || depth || bloch, "fbx_rpe_phase: no output asked for");
    return rpe_check_depths(K, "fbx_rpe_phase");
}

static int rpe_shots_check(int n_qubits, int64_t B, int K, int64_t n_shots, const void* x_bits, const void* y_bits, int col, int zcol,
                           int post_select, const void* phase, const void* depth, const void* bloch, const void* moments) {
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 8, "fbx_rpe_from_shots: n_qubits must be 1..8");
    FBX_REQUIRE(B >= 0 && K >= 1 && n_shots >= 1, "fbx_rpe_from_shots: need B >= 0, K >= 1 and n_shots >= 1");
    FBX_REQUIRE(col >= 0 && col < n_qubits, "fbx_rpe_from_shots: col must be a column of the record");
    FBX_REQUIRE(zcol >= -1 && zcol < n_qubits && zcol != col, "fbx_rpe_from_shots: zcol must be -1 or another column of the record");
    FBX_REQUIRE(post_select == 0 || post_select == 1, "fbx_rpe_from_shots: post_select must be 0 or 1");
    FBX_REQUIRE(B == 0 || (x_bits && y_bits), "fbx_rpe_from_shots: NULL bits");
    FBX_REQUIRE(phase || depth || bloch || moments, "fbx_rpe_from_shots: no output asked for");
    return rpe_check_depths(K, "fbx_rpe_from_shots");
}

static int circular_stats_check(int64_t R, int64_t B, const void* angles, const void* mean, const void* sd, const void* nan_count) {
    FBX_REQUIRE(R >= 0 && B >= 0, "fbx_circular_stats: need R >= 0 and B >= 0");
    FBX_REQUIRE(R * B == 0 || angles, "fbx_circular_stats: NULL angles");
    FBX_REQUIRE(mean || sd || nan_count, "fbx_circular_stats: no output asked for");
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_rpe_phase_dev(int64_t B, int K, const double* d_x, const double* d_y, const double* d_x_err, const double* d_y_err,
                      int errors_are_variances, const double* d_xz, const double* d_yz, const double* d_xz_err,
                      const double* d_yz_err, int post_select, double* d_phase_out, int32_t* d_depth_reached_out,
                      double* d_bloch_out) {
    FBX_TRY(rpe_phase_check(B, K, d_x, d_y, d_x_err, d_y_err, d_xz, d_yz, d_xz_err, d_yz_err, post_select, d_phase_out,
                            d_depth_reached_out, d_bloch_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const long long want = ((long long)B + 255) / 256;
    const unsigned grid = (unsigned)(want < 256 * 32 ? want : 256 * 32);
    hipLaunchKernelGGL(rpe_phase_kernel, dim3(grid), dim3(256), 0, stream(), (long long)B, K, d_x, d_y, d_x_err, d_y_err, d_xz, d_yz,
                       d_xz_err, d_yz_err, errors_are_variances ? 1 : 0, post_select, d_phase_out, (int*)d_depth_reached_out,
                       d_bloch_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_rpe_phase(int64_t B, int K, const double* x, const double* y, const double* x_err, const double* y_err,
                  int errors_are_variances, const double* xz, const double* yz, const double* xz_err, const double* yz_err,
                  int post_select, double* phase_out, int32_t* depth_reached_out, double* bloch_out) {
    FBX_TRY(rpe_phase_check(B, K, x, y, x_err, y_err, xz, yz, xz_err, yz_err, post_select, phase_out, depth_reached_out, bloch_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t n = (size_t)B * K;
    const double* src[8] = {x, y, x_err, y_err, xz, yz, xz_err, yz_err};
    HostIO io; double *din[8] = {}, *dphase, *dbloch; int32_t* ddepth;
    for (int a = 0; a < (xz ? 8 : 4); ++a) FBX_TRY(io.in(src[a], n, &din[a]));
    FBX_TRY(io.out_opt(phase_out, (size_t)B, &dphase)); FBX_TRY(io.out_opt(depth_reached_out, (size_t)B, &ddepth));
    FBX_TRY(io.out_opt(bloch_out, 2 * n, &dbloch));
    FBX_TRY(fbx_rpe_phase_dev(B, K, din[0], din[1], din[2], din[3], errors_are_variances, din[4], din[5], din[6], din[7], post_select,
                              dphase, ddepth, dbloch));
    return io.finish();
}

int fbx_rpe_from_shots_dev(int n_qubits, int64_t B, int K, int64_t n_shots, const uint8_t* d_x_bits, const uint8_t* d_y_bits,
                           int col, int zcol, int post_select, double* d_phase_out, int32_t* d_depth_reached_out,
                           double* d_bloch_out, double* d_moments_out) {
    FBX_TRY(rpe_shots_check(n_qubits, B, K, n_shots, d_x_bits, d_y_bits, col, zcol, post_select, d_phase_out, d_depth_reached_out,
                            d_bloch_out, d_moments_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    switch (n_qubits) {
#define FBX_RPE_SHOTS(NQ) case NQ: return launch_rpe_shots<NQ>(B, K, n_shots, d_x_bits, d_y_bits, col, zcol, post_select, \
                                                               d_phase_out, d_depth_reached_out, d_bloch_out, d_moments_out)
        FBX_RPE_SHOTS(1); FBX_RPE_SHOTS(2); FBX_RPE_SHOTS(3); FBX_RPE_SHOTS(4); FBX_RPE_SHOTS(5); FBX_RPE_SHOTS(6); FBX_RPE_SHOTS(7);
        FBX_RPE_SHOTS(8);
#undef FBX_RPE_SHOTS
    }
    return FBX_ERR_UNSUPPORTED;
}

int fbx_rpe_from_shots(int n_qubits, int64_t B, int K, int64_t n_shots, const uint8_t* x_bits, const uint8_t* y_bits, int col,
                       int zcol, int post_select, double* phase_out, int32_t* depth_reached_out, double* bloch_out,
                       double* moments_out) {
    FBX_TRY(rpe_shots_check(n_qubits, B, K, n_shots, x_bits, y_bits, col, zcol, post_select, phase_out, depth_reached_out, bloch_out,
                            moments_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t items = (size_t)B * K, nb = items * (size_t)n_shots * (size_t)n_qubits;
    HostIO io; uint8_t *dx, *dy; double *dphase, *dbloch, *dmom; int32_t* ddepth;
    FBX_TRY(io.in(x_bits, nb, &dx)); FBX_TRY(io.in(y_bits, nb, &dy));
    FBX_TRY(io.out_opt(phase_out, (size_t)B, &dphase)); FBX_TRY(io.out_opt(depth_reached_out, (size_t)B, &ddepth));
    FBX_TRY(io.out_opt(bloch_out, 2 * items, &dbloch)); FBX_TRY(io.out_opt(moments_out, 4 * items, &dmom));
    FBX_TRY(fbx_rpe_from_shots_dev(n_qubits, B, K, n_shots, dx, dy, col, zcol, post_select, dphase, ddepth, dbloch, dmom));
    return io.finish();
}

int fbx_circular_stats_dev(int64_t R, int64_t B, const double* d_angles, double* d_mean_out, double* d_std_out,
                           int32_t* d_nan_count_out) {
    FBX_TRY(circular_stats_check(R, B, d_angles, d_mean_out, d_std_out, d_nan_count_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const long long want = ((long long)B + 255) / 256;
    const unsigned grid = (unsigned)(want < 256 * 32 ? want : 256 * 32);
    hipLaunchKernelGGL(circular_stats_kernel, dim3(grid), dim3(256), 0, stream(), (long long)R, (long long)B, d_angles, d_mean_out,
                       d_std_out, (int*)d_nan_count_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_circular_stats(int64_t R, int64_t B, const double* angles, double* mean_out, double* std_out, int32_t* nan_count_out) {
    FBX_TRY(circular_stats_check(R, B, angles, mean_out, std_out, nan_count_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    HostIO io; double *da, *dm, *ds; int32_t* dn;
    FBX_TRY(io.in(angles, (size_t)R * B, &da));
    FBX_TRY(io.out_opt(mean_out, (size_t)B, &dm)); FBX_TRY(io.out_opt(std_out, (size_t)B, &ds));
    FBX_TRY(io.out_opt(nan_count_out, (size_t)B, &dn));
    FBX_TRY(fbx_circular_stats_dev(R, B, da, dm, ds, dn));
    return io.finish();
}

}  // extern "C"
