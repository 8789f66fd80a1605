// fbx_superop_prims.hpp -- what fbx_convert.hip, fbx_sweep.hip and fbx_superop.hip share: the device primitives on a D x D
// complex matrix (row-major, leading dimension LD, in LDS unless a `_big` form says HBM) that the conversions and the Kraus
// sweeps are made of, the tile geometry of the 3-qubit register passes, and the launchers one of the files needs from another.
// Every basis change uses the sparsity of the Pauli matrices (each vec(P_k) has d non-zero entries, all in {+-1, +-i}) instead
// of a dense D x D x D product.
#pragma once
#include "fbx_choi.hpp"

namespace fbx {

// fbx_convert.hip: the pairwise conversion of 1-5 qubits (psd_choi: see launch_convert_big)
int convert_launch(int n_qubits, int from, int to, int64_t B, const double* in, int K, double* out, bool psd_choi = false);
// fbx_sweep.hip: the 3-qubit sweep kernel; with one output it is also the conversion from at most 31 Kraus operators
int launch_sweep3_regs(int64_t B, int K, const double* kraus, const double* ptm_ref, double* choi, double* ptm, double* chi, double* fid);
// persistent grid of the 3-qubit register-pass kernels: two workgroups per CU, four rounds of the chip
constexpr int64_t S3_GRID = 2048;

// ---------------------------------------------------------------------------------------------
// device primitives on a D x D complex matrix, row-major with leading dimension LD, in LDS
// ---------------------------------------------------------------------------------------------

// vec(P_k)[c*d + r] = P_k[r][c]; non-zero iff c = r ^ x_k with value i^{ny} (-1)^{popc(c & z)}
// multiply v by i^ph
__device__ __forceinline__ cplx mul_iph(cplx v, int ph) {
    cplx o;
    switch (ph & 3) {
        case 0: o = v; break;
        case 1: o.re = -v.im; o.im = v.re; break;
        case 2: o.re = -v.re; o.im = -v.im; break;
        default: o.re = v.im; o.im = -v.re; break;
    }
    return o;
}

// out = scale * P2C^H in P2C  (superop -> Pauli-Liouville with scale 1/d; Choi -> chi with 1/d^2),
// P2C columns = vec(P_k): out[k][l] = scale * sum_{r,s} conj(vP_k[r]) in[r][s] vP_l[s]
template <int NQ, int NT = 64, int LD = (1 << (2 * NQ)) + 1>
__device__ void to_pauli_basis(const cplx* in, cplx* out, double scale, int lane) {
    constexpr int d = 1 << NQ, D = d * d;
    for (int idx = lane; idx < D * D; idx += NT) {
        const int k = idx / D, l = idx % D;
        int xk, zk, yk, xl, zl, yl;
        pauli_masks<NQ>(k, xk, zk, yk);
        pauli_masks<NQ>(l, xl, zl, yl);
        double re = 0.0, im = 0.0;
        for (int rk = 0; rk < d; ++rk) {          // row index of P_k's non-zero: (rk, ck = rk ^ xk)
            const int ck = rk ^ xk;
            const int sk = __popc(ck & zk) & 1;
#pragma unroll
            for (int rl = 0; rl < d; ++rl) {
                const int cl = rl ^ xl;
                const int sl = __popc(cl & zl) & 1;
                const cplx v = in[(ck * d + rk) * LD + cl * d + rl];
                // conj(i^yk) * i^yl = i^(yl - yk)
                const cplx w = mul_iph(v, (yl - yk) & 3);
                if (sk ^ sl) { re -= w.re; im -= w.im; } else { re += w.re; im += w.im; }
            }
        }
        cplx o; o.re = re * scale; o.im = im * scale;
        out[k * LD + l] = o;
    }
}

// out = scale * P2C in P2C^H: out[r][s] = scale * sum_{k,l} vP_k[r] in[k][l] conj(vP_l[s])
template <int NQ, int NT = 64, int LD = (1 << (2 * NQ)) + 1>
__device__ void from_pauli_basis(const cplx* in, cplx* out, double scale, int lane) {
    constexpr int d = 1 << NQ, D = d * d;
    for (int idx = lane; idx < D * D; idx += NT) {
        const int r = idx / D, s = idx % D;
        const int cr = r / d, rr = r % d, cs = s / d, rs = s % d;   // vec index = col * d + row
        const int xk = rr ^ cr, xl = rs ^ cs;
        double re = 0.0, im = 0.0;
        for (int zk = 0; zk < d; ++zk) {
            const int k = pauli_index<NQ>(xk, zk);
            const int yk = __popc(xk & zk), sk = __popc(cr & zk) & 1;
#pragma unroll
            for (int zl = 0; zl < d; ++zl) {
                const int l = pauli_index<NQ>(xl, zl);
                const int yl = __popc(xl & zl), sl = __popc(cs & zl) & 1;
                const cplx w = mul_iph(in[k * LD + l], (yk - yl) & 3);
                if (sk ^ sl) { re -= w.re; im -= w.im; } else { re += w.re; im += w.im; }
            }
        }
        cplx o; o.re = re * scale; o.im = im * scale;
        out[r * LD + s] = o;
    }
}

// Site-factored forms of the two transforms above: P2C factors over the qubits, so the change of basis
// is 2n in-place butterfly stages (one quad per thread and stage) and a bit-permuting copy instead of a
// D-term sum per entry.  Element index = row * D + col with row = (a_{n-1}..a_0 b_{n-1}..b_0) = vec
// index c*d + r; the stages pair (a_t, b_t) of the row (conj: -i) and of the column (+i); Pauli digit
// 2 a_t + b_t of label k is I, X, Y, Z, so entry [k][l] of the Pauli side sits at row site_index(k),
// column site_index(l).  The forward form destroys `in`.  NT threads, NT >= D*D/4 or a multiple loop.
template <int NQ>
__device__ __forceinline__ int site_index(int k) {
    int r = 0;
#pragma unroll
    for (int t = 0; t < NQ; ++t) r |= (((k >> (2 * t + 1)) & 1) << (NQ + t)) | (((k >> (2 * t)) & 1) << t);
    return r;
}
template <int NT>
__device__ __forceinline__ void sites_sync() { if constexpr (NT <= 64) FBX_WAVE_SYNC(); else __syncthreads(); }
template <int NQ, bool INVERSE, int NT, int LD>
__device__ __forceinline__ void site_stages(cplx* M, int t) {
    static_assert(NT >= (1 << (4 * NQ)) / 4, "one quad per thread");
#pragma unroll
    for (int q = NQ - 1; q >= 0; --q) { pauli_site_stage<NQ, INVERSE, LD>(M, t, 3 * NQ + q, 2 * NQ + q, -1.0); sites_sync<NT>(); }
#pragma unroll
    for (int q = NQ - 1; q >= 0; --q) { pauli_site_stage<NQ, INVERSE, LD>(M, t, NQ + q, q, +1.0); sites_sync<NT>(); }
}
template <int NQ, int NT = 64, int LD = (1 << (2 * NQ)) + 1>
__device__ void to_pauli_sites(cplx* in, cplx* out, double scale, int t) {
    constexpr int D = 1 << (2 * NQ);
    site_stages<NQ, false, NT, LD>(in, t);
    for (int idx = t; idx < D * D; idx += NT) {
        const int k = idx / D, l = idx % D;
        cplx v = in[site_index<NQ>(k) * LD + site_index<NQ>(l)];
        v.re *= scale; v.im *= scale;
        out[k * LD + l] = v;
    }
}
// P2C x P2C^H = D * (inverse of the forward stages)
template <int NQ, int NT = 64, int LD = (1 << (2 * NQ)) + 1>
__device__ void from_pauli_sites(const cplx* in, cplx* out, double scale, int t) {
    constexpr int D = 1 << (2 * NQ);
    const double s = scale * D;
    for (int idx = t; idx < D * D; idx += NT) {
        const int k = idx / D, l = idx % D;
        cplx v = in[k * LD + l];
        v.re *= s; v.im *= s;
        out[site_index<NQ>(k) * LD + site_index<NQ>(l)] = v;
    }
    sites_sync<NT>();
    site_stages<NQ, true, NT, LD>(out, t);
}

// choi <-> superop reshuffle (superoperator_transformations.py:267-277,351-361):
// out[(p,q)][(r,s)] = in[(s,q)][(r,p)]
template <int NQ, int NT = 64, int LD = (1 << (2 * NQ)) + 1>
__device__ void reshuffle(const cplx* in, cplx* out, int lane) {
    constexpr int d = 1 << NQ, D = d * d;
    for (int idx = lane; idx < D * D; idx += NT) {
        const int row = idx / D, col = idx % D;
        const int p = row / d, q = row % d, r = col / d, s = col % d;
        out[row * LD + col] = in[(s * d + q) * LD + r * d + p];
    }
}

// One entry of the two Kraus products, from K operators k stored row-major d x d one after the other:
//   superop = sum_t conj(K_t) (x) K_t:    [(i,k)][(j,l)] = conj(K[i][j]) K[k][l]
//   choi    = sum_t vec(K_t) vec(K_t)^H:  vec(K)[c d + r] = K[r][c];  [row][col] = vK[row] conj(vK[col])
// The conjugate is taken by a sign flip in front of a plain complex product: with -ffp-contract=on the spelling decides which
// product of each sum is fused, and this one is what every user of these entries has always computed.
template <bool CONJ_A>
__device__ __forceinline__ cplx kraus_sum(const cplx* k, int K, int D, int ia, int ib) {
    double re = 0.0, im = 0.0;
    for (int t = 0; t < K; ++t) {
        cplx a = k[(long long)t * D + ia], b = k[(long long)t * D + ib];
        if (CONJ_A) a.im = -a.im; else b.im = -b.im;
        re += a.re * b.re - a.im * b.im;
        im += a.re * b.im + a.im * b.re;
    }
    cplx o; o.re = re; o.im = im;
    return o;
}
__device__ __forceinline__ cplx kraus_superop_entry(const cplx* k, int K, int d, int row, int col) {
    return kraus_sum<true>(k, K, d * d, (row / d) * d + col / d, (row % d) * d + col % d);
}
__device__ __forceinline__ cplx kraus_choi_entry(const cplx* k, int K, int d, int row, int col) {
    return kraus_sum<false>(k, K, d * d, (row % d) * d + row / d, (col % d) * d + col / d);
}

// kraus -> choi or superop; K ops row-major d x d in HBM
template <int NQ, int NT = 64, int LD = (1 << (2 * NQ)) + 1>
__device__ void kraus_to(const double* __restrict__ kraus, int K, bool to_superop, cplx* out, cplx* kb,
                         int lane) {
    constexpr int d = 1 << NQ, D = d * d;
    for (int idx = lane; idx < K * D; idx += NT) { kb[idx].re = kraus[2 * idx]; kb[idx].im = kraus[2 * idx + 1]; }
    __syncthreads();
    for (int idx = lane; idx < D * D; idx += NT) {
        const int row = idx / D, col = idx % D;
        out[row * LD + col] = to_superop ? kraus_superop_entry(kb, K, d, row, col) : kraus_choi_entry(kb, K, d, row, col);
    }
}

// matrix absolute value through the eigendecomposition, as choi2kraus -> kraus2choi does it
// (superoperator_transformations.py:325-336): numpy eigh reads the LOWER triangle; eigenvalues
// with |lambda| <= tol are dropped; sqrt of a negative eigenvalue is imaginary, so the rebuilt
// matrix is sum |lambda| v v^H.
template <int NQ>
__device__ void abs_via_eigh(const cplx* in, cplx* out, ChoiLds<NQ>& L, double tol, int lane) {
    constexpr int d = 1 << NQ, D = d * d, LD = D + 1, NB = D / 2;
    Blk h = blk_zero();
    if (lane < NB * NB) {
        const int I = lane / NB, J = lane % NB;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 2 * I + (e >> 1), c = 2 * J + (e & 1);
            if (r > c) { const cplx v = in[r * LD + c]; h.re[e] = v.re; h.im[e] = v.im; }
            else if (r < c) { const cplx v = in[c * LD + r]; h.re[e] = v.re; h.im[e] = -v.im; }
            else { h.re[e] = in[r * LD + c].re; h.im[e] = 0.0; }
        }
    }
    __syncthreads();
    sys_store<D>(L.Ms, lane, h);
    __syncthreads();
    jacobi_eigh_lds<D>(L.Ms, L.Vs, L.rec, lane);
    if (lane < D) {
        const double l = fabs(L.Ms[sys_index<D>(lane, lane)].re);
        L.lam[lane] = l > tol ? l : 0.0;
    }
    __syncthreads();
    const Blk a = reconstruct_blk<D>(L.Vs, L.lam, lane);
    blk_store<D, LD>(out, lane, a);
    __syncthreads();
}

template <int NQ, int NT = 64, int LD = (1 << (2 * NQ)) + 1>
__device__ void load_matrix(const double* __restrict__ g, cplx* m, int lane) {
    constexpr int d = 1 << NQ, D = d * d;
    for (int idx = lane; idx < D * D; idx += NT) {
        cplx v; v.re = g[2 * idx]; v.im = g[2 * idx + 1];
        m[(idx / D) * LD + idx % D] = v;
    }
}
template <int NQ, int NT = 64, int LD = (1 << (2 * NQ)) + 1>
__device__ void store_matrix(const cplx* m, double* __restrict__ g, int lane) {
    constexpr int d = 1 << NQ, D = d * d;
    for (int idx = lane; idx < D * D; idx += NT) {
        const cplx v = m[(idx / D) * LD + idx % D];
        g[2 * idx] = v.re; g[2 * idx + 1] = v.im;
    }
}

// ---------------------------------------------------------------------------------------------
// 4 and 5 qubits (256 x 256 / 1024 x 1024 superoperators): the same walk through the representation graph
// with the two work matrices of an item in HBM / L2 (1 MB / 16 MB each) instead of LDS -- one 1024-thread
// workgroup per item, every primitive looped over the entries (or the quads of a butterfly stage) with a
// workgroup barrier between the stages.  Conversions INTO chi from anything but Kraus operators go through
// a D x D eigendecomposition in the reference (choi2kraus) and are not offered beyond 3 qubits.
// ---------------------------------------------------------------------------------------------
template <int NQ, bool INVERSE, int NT>
__device__ void site_stages_big(cplx* M, int t) {
    constexpr int D = 1 << (2 * NQ), NQUAD = D * D / 4;
#pragma unroll 1
    for (int q = NQ - 1; q >= 0; --q) {
        for (int u = t; u < NQUAD; u += NT) pauli_site_stage<NQ, INVERSE, D>(M, u, 3 * NQ + q, 2 * NQ + q, -1.0);
        __syncthreads();
    }
#pragma unroll 1
    for (int q = NQ - 1; q >= 0; --q) {
        for (int u = t; u < NQUAD; u += NT) pauli_site_stage<NQ, INVERSE, D>(M, u, NQ + q, q, +1.0);
        __syncthreads();
    }
}
template <int NQ, int NT>
__device__ void to_pauli_big(cplx* in, cplx* out, double scale, int t) {        // destroys `in`
    constexpr int D = 1 << (2 * NQ);
    site_stages_big<NQ, false, NT>(in, t);
    for (int idx = t; idx < D * D; idx += NT) {
        cplx v = in[site_index<NQ>(idx / D) * D + site_index<NQ>(idx % D)];
        v.re *= scale; v.im *= scale;
        out[idx] = v;
    }
}
template <int NQ, int NT>
__device__ void from_pauli_big(const cplx* in, cplx* out, double scale, int t) {
    constexpr int D = 1 << (2 * NQ);
    const double s = scale * D;
    for (int idx = t; idx < D * D; idx += NT) {
        cplx v = in[idx];
        v.re *= s; v.im *= s;
        out[site_index<NQ>(idx / D) * D + site_index<NQ>(idx % D)] = v;
    }
    __syncthreads();
    site_stages_big<NQ, true, NT>(out, t);
}

// results of the sweep are written once and never re-read by the kernel: stream them past the caches
typedef double fbx_d2v __attribute__((ext_vector_type(2)));
#define FBX_STREAM_STORE(ptr, val) __builtin_nontemporal_store(fbx_d2v{(val).x, (val).y}, reinterpret_cast<fbx_d2v*>(ptr))

// two sites on the 16 registers of a lane: register index r = (p1 q1 p2 q2); (I, Z, X, Y) end up at / start from
// (00, 11, 01, 10).  The inverse butterflies run in the same order (the stages commute).
template <bool INVERSE = false>
__device__ __forceinline__ void two_sites(cplx (&x)[16], double y1, double y2) {
    auto site = [](cplx& c00, cplx& c11, cplx& c01, cplx& c10, double ys) {
        if constexpr (!INVERSE) {
            cplx oi, oz, ox, oy;
            oi.re = c00.re + c11.re; oi.im = c00.im + c11.im;
            oz.re = c00.re - c11.re; oz.im = c00.im - c11.im;
            ox.re = c01.re + c10.re; ox.im = c01.im + c10.im;
            const double dr = c01.re - c10.re, di = c01.im - c10.im;
            oy.re = -ys * di; oy.im = ys * dr;
            c00 = oi; c11 = oz; c01 = ox; c10 = oy;
        } else {
            cplx o00, o11, o01, o10;
            o00.re = 0.5 * (c00.re + c11.re); o00.im = 0.5 * (c00.im + c11.im);
            o11.re = 0.5 * (c00.re - c11.re); o11.im = 0.5 * (c00.im - c11.im);
            const double yr = -ys * c10.im, yi = ys * c10.re;                      // s * i * Y
            o01.re = 0.5 * (c01.re - yr); o01.im = 0.5 * (c01.im - yi);
            o10.re = 0.5 * (c01.re + yr); o10.im = 0.5 * (c01.im + yi);
            c00 = o00; c11 = o11; c01 = o01; c10 = o10;
        }
    };
#pragma unroll
    for (int cd = 0; cd < 4; ++cd) site(x[cd], x[12 | cd], x[4 | cd], x[8 | cd], y1);            // p1 = bit 3, q1 = bit 2
#pragma unroll
    for (int ab = 0; ab < 4; ++ab) site(x[ab << 2], x[(ab << 2) | 3], x[(ab << 2) | 1], x[(ab << 2) | 2], y2);   // p2 = bit 1, q2 = bit 0
}

// Three qubits, fused, two butterfly stages per pass in REGISTERS (round 4, second form; the kernel above stays as the A/B and
// as the form for FBX_SWEEP3_V1=1).  The first form did one stage per pass through LDS: per transform and thread 28 ds_write_b128
// (13 cycles each) + 60 ds_read_b128, 19 k LDS-pipe cycles per item against 15 k cycles of HBM time per item and CU -- LDS-bound
// (3.5-3.8 TB/s, 31 % bank conflicts).  Here a workgroup is 256 threads, a thread holds a 4 x 4 sub-tile (16 entries = two bit
// pairs of the 12-bit element index, as the 2-qubit kernel's two_sites) and the six stages are three passes:
//   P1  row site 2 + column site 2   registers = row bits {5,2} x column bits {5,2}: the tile is BUILT here from the Kraus operators
//                                    (4 + 4 operator entries per Kraus operator for 16 products), the Choi matrix leaves from here
//   P2  column sites 1 and 0         registers = column bits {4,1,3,0}, in place
//   P3  row sites 1 and 0            registers = row bits {4,1,3,0} = the output row's low four bits, lanes = the 64 output
//                                    columns: every store instruction of a wavefront writes one whole 1 KB output row
// Two LDS round trips (32 writes + 32 reads of 16 B per thread) + 32 broadcast reads of the operators: 5 k LDS-pipe cycles per
// item.  Layout X[row][col ^ g(row)], g(row) = r1 | r3 << 1 | r0 << 2 | r4 << 3, with the thread bits of every pass assigned so
// that each ds_write_b128 lane group (8 contiguous lanes, 128-B bank period) and each ds_read_b128 lane group (the four
// non-contiguous 16-lane groups of MI355X_MICROARCH.md, 256-B period) touches distinct 16-byte slots:
//   P1 threads  l0 l1 l2 l3 l4 l5 w0 w1 -> c0 c1 r0 c3 c4 r1 r3 r4
//   P2 threads                          -> c2 r1 r3 c5 r4 r0 r2 r5
//   P3 threads                          -> c0 c3 c1 c4 c2 c5 r2 r5   (lane = output column: column bit t = l bit 2t, 3 + t = 2t + 1)
// The stages commute (each acts on its own pair of index bits), so the grouping by site changes rounding only.
__device__ __forceinline__ int s3_swz(int row) { return ((row >> 1) & 1) | (((row >> 3) & 1) << 1) | ((row & 1) << 2) | (((row >> 4) & 1) << 3); }
__device__ __forceinline__ int s3_addr(int row, int col) { return row * 64 + (col ^ s3_swz(row)); }

// The geometry above for thread t of a 256-thread workgroup.  LDS address of register r in a pass = the thread's base XOR a
// compile-time constant: the register bits are disjoint from the thread bits, and the swizzle of a row depends on thread bits
// only (P1, P2) or on register bits only (P3).  The bases are re-made opaque where they are used, so that the compiler keeps
// three of them across the item loop and not 48 addresses.
struct S3Tile {
    int row1, col1, row2, col2, row3, col3;      // thread bits -> element bits of the three passes; the register part is added per register
    int lcol, krow;                              // output column / first output row of P3
    int base1, base2, base3;
    __device__ __forceinline__ explicit S3Tile(int t) {
        auto bit = [](int v, int b) { return (v >> b) & 1; };
        const int w0 = bit(t, 6), w1 = bit(t, 7);
        row1 = bit(t, 2) | bit(t, 5) << 1 | w0 << 3 | w1 << 4;                       // P1: r0 r1 r3 r4
        col1 = bit(t, 0) | bit(t, 1) << 1 | bit(t, 3) << 3 | bit(t, 4) << 4;           //     c0 c1 c3 c4
        row2 = bit(t, 5) | bit(t, 1) << 1 | w0 << 2 | bit(t, 2) << 3 | bit(t, 4) << 4 | w1 << 5;   // P2: all six row bits
        col2 = bit(t, 0) << 2 | bit(t, 3) << 5;                                        //     c2 c5
        row3 = w0 << 2 | w1 << 5;                                                      // P3: r2 r5
        col3 = bit(t, 0) | bit(t, 2) << 1 | bit(t, 4) << 2 | bit(t, 1) << 3 | bit(t, 3) << 4 | bit(t, 5) << 5;
        lcol = t & 63; krow = (t >> 6) * 16;
        base1 = s3_addr(row1, col1); base2 = s3_addr(row2, col2); base3 = row3 * 64 + col3;
    }
    // register r = (b3 b2 b1 b0) of a pass -> its row / column offset
    static __device__ __forceinline__ int reg_row1(int r) { return ((r >> 3) & 1) << 5 | ((r >> 2) & 1) << 2; }          // P1: b3 = r5, b2 = r2
    static __device__ __forceinline__ int reg_col1(int r) { return ((r >> 1) & 1) << 5 | (r & 1) << 2; }                 //     b1 = c5, b0 = c2
    static __device__ __forceinline__ int reg_col2(int r) { return ((r >> 3) & 1) << 4 | ((r >> 2) & 1) << 1 | ((r >> 1) & 1) << 3 | (r & 1); }   // P2: c4 c1 c3 c0
    static __device__ __forceinline__ int reg_row3(int r) { return reg_col2(r); }                                        // P3: r4 r1 r3 r0
    // the tile of P1 leaves the registers
    __device__ __forceinline__ void store1(cplx* X, const cplx (&x)[16]) const {
        const int b1 = opaque(base1);
#pragma unroll
        for (int r = 0; r < 16; ++r) X[b1 ^ (reg_row1(r) * 64 + reg_col1(r))] = x[r];
    }
    // passes 2 and 3 on the tile P1 left in X: sites(x, y1, y2) is the butterfly pair, out(r, x[r]) takes register r of P3
    template <class Sites, class Out>
    __device__ __forceinline__ void passes23(cplx* X, Sites sites, Out out) const {
        cplx x[16];
        const int b2 = opaque(base2);
#pragma unroll
        for (int r = 0; r < 16; ++r) x[r] = X[b2 ^ reg_col2(r)];
        sites(x, +1.0, +1.0);                              // column sites 1, 0 (output qubits: +i)
#pragma unroll
        for (int r = 0; r < 16; ++r) X[b2 ^ reg_col2(r)] = x[r];
        __syncthreads();
        const int b3 = opaque(base3);
#pragma unroll
        for (int r = 0; r < 16; ++r) x[r] = X[b3 ^ (reg_row3(r) * 64 + s3_swz(reg_row3(r)))];
        sites(x, -1.0, -1.0);                              // row sites 1, 0 (input qubits: -i)
#pragma unroll
        for (int r = 0; r < 16; ++r) out(r, x[r]);
    }
};

}  // namespace fbx
