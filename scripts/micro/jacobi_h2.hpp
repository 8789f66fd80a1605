// scripts/micro/jacobi_bench.hip -DFBX_JACOBI_H2 includes this file: the single-wavefront 16 x 16 solver with two workers per upper
// block (the HERMITIAN SYMMETRY of the work matrix used without idling a lane), in isolation.  Round 5 developed the form here; it
// has since become JacobiWave<N, true> of csrc/fbx_eigh.hpp (the description is there), and a copy kept here stopped compiling when
// the library moved on.  So this file forwards to the library's loop: the micro-benchmark measures the shipped round, whatever
// that is.  Build with -mllvm -amdgpu-sched-strategy=max-ilp, as fbx_pgdb.hip is (jacobi_bench_h2_ilp).
#pragma once
namespace fbx {
template <int N>
__device__ int jacobi_eigh_wave_h2(cplx* __restrict__ Ms, cplx* __restrict__ Vs, int lane, bool init_identity,
                                   double expect_n2 = -1.0, double tol2 = FBX_JACOBI_TOL2) {
    return JacobiWave<N, true>::run(Ms, Vs, lane, init_identity, expect_n2, tol2);
}
}  // namespace fbx
