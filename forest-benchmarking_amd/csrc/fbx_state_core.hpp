// fbx_state_core.hpp -- what the state estimators (fbx_state.hip) and the work after a reconstruction (fbx_state_measures.hip) share:
// the LDS of the one-wavefront kernels, the Pauli passes and their per-lane tables, the TEAMS (how the threads that share one
// d x d state sum and synchronise) and, written once over a team, the matrix product and the Hermitian matrix function.
// Thread t of a team owns matrix entry (t / d, t % d) of its state.
#pragma once
#include "fbx_eigh64.hpp"
#include <cfloat>
#include <cmath>
#include <type_traits>

namespace fbx {

template <int NQ>
struct StateLds {
    static constexpr int d = 1 << NQ, D = d * d;
    cplx *rho, *U, *tmp, *aux;     // [d*d] row-major
    cplx *Ms, *Vs;                 // [d*d] Jacobi layout
    JRec* rec;                     // [d/2 + 1]
    double *w, *r, *lam;           // [D], [D], [d]
    double *hs, *hd;               // [m] per-setting scratch
    __host__ __device__ static constexpr size_t bytes(int m) {
        return sizeof(cplx) * 6 * D + sizeof(JRec) * (d / 2 + 1) + sizeof(double) * (2 * D + d + 2 * (size_t)m) + 64;
    }
    // The per-setting scratch (16 bytes per setting) is staged in LDS up to 64 KiB; a design beyond that -- a state-tomography
    // dataset repeated or merged some 60 times over -- takes the streamed form of r_operator_strided (fbx_state.hip), which needs none.
    __host__ __device__ static constexpr bool staged(int m) { return bytes(m) <= 64 * 1024; }
    __host__ __device__ static constexpr size_t launch_bytes(int m) { return bytes(staged(m) ? m : 0); }
    __device__ void carve(char* p, int m) {
        rho = (cplx*)p; p += sizeof(cplx) * D;  U = (cplx*)p; p += sizeof(cplx) * D;
        tmp = (cplx*)p; p += sizeof(cplx) * D;  aux = (cplx*)p; p += sizeof(cplx) * D;
        Ms = (cplx*)p; p += sizeof(cplx) * D;   Vs = (cplx*)p; p += sizeof(cplx) * D;
        rec = (JRec*)p; p += sizeof(JRec) * (d / 2 + 1);
        w = (double*)p; p += sizeof(double) * D; r = (double*)p; p += sizeof(double) * D;
        lam = (double*)p; p += sizeof(double) * d;
        hs = (double*)p; p += sizeof(double) * m; hd = (double*)p;
    }
};

// P_p[row][row ^ x] = i^{ny} (-1)^{popc((row ^ x) & z)}
__device__ __forceinline__ void pauli_entry(int x, int z, int ny, int row, int& col, int& ph, int& neg) {
    col = row ^ x; ph = ny & 3; neg = __popc(col & z) & 1;
}

// r[p] = Re tr(P_p rho) for every Pauli index p (lanes p < D)
template <int NQ>
__device__ void pauli_expectations(const cplx* rho, double* r, int lane) {
    constexpr int d = 1 << NQ, D = d * d;
    if (lane < D) {
        int x, z, ny; pauli_masks<NQ>(lane, x, z, ny);
        double acc = 0.0;
#pragma unroll
        for (int row = 0; row < d; ++row) {
            int col, ph, neg; pauli_entry(x, z, ny, row, col, ph, neg);
            const cplx v = rho[col * d + row];                 // rho[col][row]
            const double t = (ph == 0) ? v.re : (ph == 1) ? -v.im : (ph == 2) ? -v.re : v.im;
            acc += neg ? -t : t;
        }
        r[lane] = acc;
    }
}

// element (row, col) of  w0 * I + sum_p w[p] P_p
template <int NQ>
__device__ __forceinline__ cplx pauli_synthesis(const double* w, double w0, int row, int col) {
    constexpr int d = 1 << NQ;
    const int x = row ^ col;
    double re = (row == col) ? w0 : 0.0, im = 0.0;
#pragma unroll
    for (int z = 0; z < d; ++z) {
        const int p = pauli_index<NQ>(x, z);
        const int ph = __popc(x & z) & 3, neg = __popc(col & z) & 1;
        double v = w[p]; v = neg ? -v : v;
        if (ph == 0) re += v; else if (ph == 1) im += v; else if (ph == 2) re -= v; else im -= v;
    }
    cplx o; o.re = re; o.im = im; return o;
}

// Round 6: the two Pauli passes of the iterative-MLE loop with their per-lane index and sign logic evaluated ONCE per reconstruction.
// The state kernels are bound by vector-instruction issue (profiles/r06: 46-48 % of their vector instructions are fp64 arithmetic,
// the rest phase selects, index arithmetic and reductions), and what a lane selects in pauli_expectations / pauli_synthesis depends on
// nothing but the lane: lane p reads the SAME component (real or imaginary, by the number of Y factors of its Pauli) of d fixed
// entries with fixed signs; entry (row, col) adds d fixed weights with fixed signs to its real or imaginary part.  As tables: one
// 8-byte LDS read + one FMA with a +-1 constant per term (expectations), one read + two FMAs with constants in {0, +-1} (synthesis).
// A product with +-1 is exact and a term with coefficient 0 leaves a non-negative-zero accumulator untouched: BIT-IDENTICAL to the
// select forms above (tests/test_state_gpu.py holds both against the reference fixtures; scripts/compare_libs.py the hashes).
template <int NQ>
struct PauliTables {
    static constexpr int d = 1 << NQ;
    int eoff[d]; double esg[d];             // r[p] = sum_row esg[row] * ((double*)rho)[eoff[row]]
    int sp[d]; double sa[d], sb[d];         // entry: re += sa[z] * w[sp[z]], im += sb[z] * w[sp[z]]
    // lane `p` of the expectation pass, entry (row, col) of the synthesis pass
    __device__ __forceinline__ void init(int p, int row, int col) {
        int x, z, ny; pauli_masks<NQ>(p, x, z, ny);
#pragma unroll
        for (int r = 0; r < d; ++r) {
            int c, ph, neg; pauli_entry(x, z, ny, r, c, ph, neg);
            const double s = neg ? -1.0 : 1.0;
            eoff[r] = 2 * (c * d + r) + (ph & 1);                               // ph 0 / 2: real part, 1 / 3: imaginary part
            esg[r] = (ph == 0 || ph == 3) ? s : -s;
        }
        const int xs = row ^ col;
#pragma unroll
        for (int zz = 0; zz < d; ++zz) {
            sp[zz] = pauli_index<NQ>(xs, zz);
            const int ph = __popc(xs & zz) & 3, neg = __popc(col & zz) & 1;
            const double s = neg ? -1.0 : 1.0;
            sa[zz] = ph == 0 ? s : ph == 2 ? -s : 0.0;
            sb[zz] = ph == 1 ? s : ph == 3 ? -s : 0.0;
        }
    }
    __device__ __forceinline__ double expectation(const cplx* rho) const {
        const double* f = reinterpret_cast<const double*>(rho);
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < d; ++r) acc = fma(esg[r], f[eoff[r]], acc);
        return acc;
    }
    __device__ __forceinline__ cplx synthesis(const double* w, double w0, bool on_diagonal) const {
        double re = on_diagonal ? w0 : 0.0, im = 0.0;
#pragma unroll
        for (int zz = 0; zz < d; ++zz) { const double v = w[sp[zz]]; re = fma(sa[zz], v, re); im = fma(sb[zz], v, im); }
        cplx o; o.re = re; o.im = im; return o;
    }
};

// The same tables with ONE +-1.0 sign per term (d doubles per pass instead of 2 d coefficients) and the synthesis terms ordered by the part
// they feed: what the 3-qubit kernel uses -- with the coefficients above it holds 236 registers (two wavefronts per SIMD),
// with these 110 (four).  Entry (row, col), x = row ^ col: the weights with even popc(x & z) feed the real part, those with odd parity the
// imaginary part -- for x != 0 half of the z each, in ascending z inside each half; on the diagonal (x = 0) all d feed the real part.  The
// list holds the real-part terms first, in ascending z, then the others: the first d / 2 terms always go to the real accumulator, the
// second half continues the SAME accumulator on the diagonal and starts the imaginary one elsewhere, so every sum keeps the order of the
// select form (bit-identical).
template <int NQ>
struct PauliTablesLean {
    static constexpr int d = 1 << NQ;
    int eoff[d]; double esg[d];             // r[p] = sum_row esg[row] * ((double*)rho)[eoff[row]], esg = +-1
    int sp[d]; double ssg[d];               // synthesis term k: ssg[k] * w[sp[k]], ssg = +-1
    __device__ __forceinline__ void init(int p, int row, int col) {
        int x, z, ny; pauli_masks<NQ>(p, x, z, ny);
        unsigned esign = 0u, ssign = 0u;        // bit r: the expectation term of row r enters negated; bit k: synthesis term k does
#pragma unroll
        for (int r = 0; r < d; ++r) {
            int c, ph, neg; pauli_entry(x, z, ny, r, c, ph, neg);
            eoff[r] = 2 * (c * d + r) + (ph & 1);
            const bool minus = (ph == 0 || ph == 3) ? neg != 0 : neg == 0;
            esign |= (minus ? 1u : 0u) << r;
        }
        const int xs = row ^ col;
#pragma unroll
        for (int q = 0; q < d; ++q) sp[q] = 0;
        int k = 0;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int zz = 0; zz < d; ++zz) {
                const int ph = __popc(xs & zz) & 3, neg = __popc(col & zz) & 1;
                if ((ph & 1) == pass) {
                    const bool minus = (ph >= 2) != (neg != 0);
                    // (k is a compile-time-unknown position: the writes below are selects over the d slots, once per reconstruction)
                    const int pidx = pauli_index<NQ>(xs, zz);
#pragma unroll
                    for (int q = 0; q < d; ++q) sp[q] = (q == k) ? pidx : sp[q];
                    ssign |= (minus ? 1u : 0u) << k;
                    ++k;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < d; ++q) { esg[q] = ((esign >> q) & 1u) ? -1.0 : 1.0; ssg[q] = ((ssign >> q) & 1u) ? -1.0 : 1.0; }
    }
    __device__ __forceinline__ double expectation(const cplx* rho) const {
        const double* f = reinterpret_cast<const double*>(rho);
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < d; ++r) acc = fma(esg[r], f[eoff[r]], acc);
        return acc;
    }
    __device__ __forceinline__ cplx synthesis(const double* w, double w0, bool on_diagonal) const {
        double re = on_diagonal ? w0 : 0.0;
#pragma unroll
        for (int k = 0; k < d / 2; ++k) re = fma(ssg[k], w[sp[k]], re);
        double acc = on_diagonal ? re : 0.0;                  // the diagonal continues its real sum, every other entry starts the imaginary one
#pragma unroll
        for (int k = d / 2; k < d; ++k) acc = fma(ssg[k], w[sp[k]], acc);
        cplx o; o.re = on_diagonal ? acc : re; o.im = on_diagonal ? 0.0 : acc; return o;
    }
};

// v / tr for a complex trace (tr_re, tr_im)
__device__ __forceinline__ cplx div_by_trace(const cplx v, double tr_re, double tr_im) {
    const double den = tr_re * tr_re + tr_im * tr_im;
    cplx q; q.re = (v.re * tr_re + v.im * tr_im) / den; q.im = (v.im * tr_re - v.re * tr_im) / den;
    return q;
}

// f(lambda) of herm_function: fn 0: log, 1: pseudo-inverse (lmax = the largest |lambda|), 2: sqrt(max(., 0))
template <int d>
__device__ __forceinline__ double spectral_function(int fn, double l, double lmax) {
    if (fn == 0) return log(l);
    if (fn == 1) return (fabs(l) > d * DBL_EPSILON * lmax) ? 1.0 / l : 0.0;   // scipy pinv cut-off
    return sqrt(l > 0.0 ? l : 0.0);
}

// block t of the Hermitian matrix in the lower triangle of row-major `src` (what scipy / numpy eigh read)
template <int d>
__device__ __forceinline__ Blk lower_blk(const cplx* src, int t) {
    constexpr int NB = d / 2;
    const int I = t / NB, J = t % NB;
    Blk h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 2 * I + (e >> 1), c = 2 * J + (e & 1);
        const cplx v = r >= c ? src[r * d + c] : src[c * d + r];
        h.re[e] = v.re;
        h.im[e] = r > c ? v.im : r < c ? -v.im : 0.0;
    }
    return h;
}
// block t of the Hermitian part of row-major `src`
template <int d>
__device__ __forceinline__ Blk herm_part_blk(const cplx* src, int t) {
    constexpr int NB = d / 2;
    const int I = t / NB, J = t % NB;
    Blk h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 2 * I + (e >> 1), c = 2 * J + (e & 1);
        const cplx a = src[r * d + c], b = src[c * d + r];
        h.re[e] = 0.5 * (a.re + b.re); h.im[e] = 0.5 * (a.im - b.im);
    }
    return h;
}

// ---- Teams.  sum(): every thread receives the total, added in one fixed order, and what the team wrote to LDS before it is visible
// after it.  sync(): the team's barrier -- between the lanes of one wavefront, which run in lockstep, a compiler fence.  Thread t of a
// team (the lane, the lane within its group, the thread of the workgroup) is passed next to the team.
template <int D>
__device__ __forceinline__ double group_sum(double v) {          // sum over the D lanes of a group, in every lane
    v += dpp_permute<0xB1>(v);                                   // quad_perm [1,0,3,2]
    v += dpp_permute<0x4E>(v);                                   // quad_perm [2,3,0,1]
    if constexpr (D == 16) { v += dpp_permute<0x141>(v); v += dpp_permute<0x140>(v); }
    return v;
}
template <int NQ>
struct WaveTeam {                   // a 64-lane wavefront per state (1-3 qubits), lanes t < D active
    static constexpr int d = 1 << NQ, D = d * d, NT = 64;
    __device__ __forceinline__ bool active(int t) const { return t < D; }
    __device__ __forceinline__ bool diag(int t) const { return t < D && t / d == t % d; }
    __device__ __forceinline__ double sum(double v) const { v = wave_sum(v); FBX_WAVE_SYNC(); return v; }
    __device__ __forceinline__ void sync() const { FBX_WAVE_SYNC(); }
    __device__ __forceinline__ double* red() const { return nullptr; }
};
template <int NQ>
struct GroupTeam {                  // D consecutive lanes of a wavefront (1-2 qubits, several states per wavefront), t = lane % D
    static constexpr int d = 1 << NQ, D = d * d, NT = D;
    __device__ __forceinline__ bool active(int) const { return true; }
    __device__ __forceinline__ bool diag(int t) const { return t / d == t % d; }
    __device__ __forceinline__ double sum(double v) const { v = group_sum<D>(v); FBX_WAVE_SYNC(); return v; }
    __device__ __forceinline__ void sync() const { FBX_WAVE_SYNC(); }
};
template <int NQ>
struct BlockTeam {                  // a workgroup of D threads per state (4-5 qubits); `scratch`: the NT / 64 doubles of LDS block_sum needs
    static constexpr int d = 1 << NQ, D = d * d, NT = D;
    double* scratch;
    __device__ __forceinline__ bool active(int) const { return true; }
    __device__ __forceinline__ bool diag(int t) const { return t / d == t % d; }
    __device__ __forceinline__ double sum(double v) const { return block_sum<NT>(v, scratch); }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ double* red() const { return scratch; }
};

// this thread's entry of A * Bm (row-major d x d); 0 in a thread without an entry
template <class Team>
__device__ __forceinline__ cplx team_matmul(const Team& tm, int t, const cplx* A, const cplx* Bm) {
    constexpr int d = Team::d, UNROLL = d <= 8 ? d : 8;     // (the factors the kernels were tuned with)
    cplx o; o.re = 0.0; o.im = 0.0;
    if (tm.active(t)) {
        const int r = t / d, c = t % d;
#pragma unroll UNROLL
        for (int k = 0; k < d; ++k) {
            const cplx a = A[r * d + k], b = Bm[k * d + c];
            o.re += a.re * b.re - a.im * b.im;
            o.im += a.re * b.im + a.im * b.re;
        }
    }
    return o;
}

// Hermitian function of a d x d matrix staged row-major in `src`: dst = V f(lambda) V^H with f selected by `fn`
// (spectral_function); eigenvalues left in L.lam.  The matrix is the lower triangle of `src` (LOWER_ONLY: what scipy / numpy eigh
// read) or its Hermitian part.  L: StateLds or StateBigLds (Ms, Vs, lam).
template <bool LOWER_ONLY, class Team, class Lds>
__device__ void herm_function(const Team& tm, int t, const cplx* src, cplx* dst, int fn, Lds& L) {
    constexpr int d = Team::d, NB = d / 2;
    Blk h = blk_zero();
    if (t < NB * NB) h = LOWER_ONLY ? lower_blk<d>(src, t) : herm_part_blk<d>(src, t);
    tm.sync();
    sys_store<d>(L.Ms, t, h);
    tm.sync();
    jacobi_eigh_simple<d, Team::NT>(L.Ms, L.Vs, t, true, tm.red());
    tm.sync();
    double lmax = 0.0;
    if (t < d) lmax = fabs(L.Ms[sys_index<d>(t, t)].re);
    lmax = wave_max(lmax);                                   // d <= 32: the diagonal sits in the first wavefront
    if (t < d) L.lam[t] = spectral_function<d>(fn, L.Ms[sys_index<d>(t, t)].re, lmax);
    tm.sync();
    const Blk o = reconstruct_blk<d>(L.Vs, L.lam, t);
    blk_store<d, d>(dst, t, o);
    tm.sync();
}

// f(std::integral_constant<int, n>()) for a number of qubits 1..5 that the caller has checked: the kernels take it as a template argument
template <class F>
int with_qubits(int n, F&& f) {
    switch (n) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        default: return f(std::integral_constant<int, 5>());
    }
}

}  // namespace fbx
