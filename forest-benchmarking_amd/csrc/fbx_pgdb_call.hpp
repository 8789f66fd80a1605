// fbx_pgdb_call.hpp -- one PGDB process-tomography call as a record, from the API to the kernel launch, and the stage plan of
// the pipelined host-pointer entry point.  Nothing from HIP in here: tests/host_harness compiles it with the host compiler
// (tests/test_pgdb_call_host.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct fbx_design;
struct ihipStream_t;        // hipStream_t is a pointer to it

namespace fbx {

// The arguments of fbx_pgdb_process_ex[_dev] for items [0, B) of the arrays it points to.  Every function between the entry
// points and the launches takes one; "items [b0, b0 + nb) of this call" is slice(b0, nb), the only place that knows the
// per-item strides.  The pointers are all device or all host pointers (the host-pointer entry point holds one of each).
struct PgdbCall {
    const fbx_design* des = nullptr;
    int64_t B = 0;
    const double* e = nullptr;     // [B][m] expectations
    const double* c = nullptr;     // [B][m] counts
    int tp = 0, mode = 0, max_iters = 0;      // mode: with FBX_MODE_LS_REFERENCE until a kernel family's dispatcher peels it off
    double* choi = nullptr;        // [B][D][D][2]
    int32_t* it = nullptr;         // [B]; this and the outputs below may be NULL
    int32_t* dy = nullptr;         // [B]
    int32_t* bt = nullptr;         // [B]
    double* cost = nullptr;        // [B]
    int32_t* sw = nullptr;         // [B][4]
    // beyond fbx_pgdb_process
    double eig_rel_tol = -1.0;     // < 0: the process default (fbx_set_option)
    int32_t* trace = nullptr;      // [B][trace_iters][2]: Dykstra iterations and halvings of every outer iteration
    int trace_iters = 0;
    // set by the pipelined host-pointer entry point only: the stream a stage's kernels go to, and the stage's share of
    // the per-item workspace: `ws_items` slots in all, this stage's start at `ws_offset` (stages on different streams get disjoint ranges)
    ihipStream_t* launch_stream = nullptr;
    int64_t ws_items = 0, ws_offset = 0;
    int64_t total_batch = 0;       // size of the caller's whole batch when this call is one block or stage of it: kernels are chosen by
                                   // IT, so that a result never depends on how a batch was cut
    size_t m = 0, DD = 0;          // strides, read from the design once (pgdb_prepare): settings, and D * D entries of a Choi matrix

    // the same call for items [b0, b0 + nb): a NULL output stays NULL, everything that is not per item is carried as it is
    PgdbCall slice(int64_t b0, int64_t nb) const {
        PgdbCall s = *this;
        const size_t o = (size_t)b0;
        s.B = nb;
        s.e = at(e, o * m); s.c = at(c, o * m);
        s.choi = at(choi, o * DD * 2);
        s.it = at(it, o); s.dy = at(dy, o); s.bt = at(bt, o); s.cost = at(cost, o);
        s.sw = at(sw, o * 4);
        s.trace = at(trace, o * (size_t)trace_iters * 2);
        return s;
    }

private:
    template <class T> static T* at(T* p, size_t offset) { return p ? p + offset : nullptr; }
};

// The stages of the pipelined host-pointer entry point (pgdb_host_pipelined, fbx_pgdb.hip) for a batch of B > host_chunk items
// in page-locked buffers: H2D, kernels and D2H overlap on separate streams (SURVEY.md 8d prices the path including both
// transfers).  What cannot be hidden is the H2D of the first stage and the D2H of the last, and every boundary between stages
// costs a launch tail (a stage's slowest items run while SIMDs idle): so the plan is a SMALL first stage
// (fbx_set_option("pgdb_host_chunk") items, default 4096 = two reconstructions per wave slot of the two-waves kernel, which runs
// them in pieces; at most half the batch), a small last one -- only when the bulk outlasts both --, and everything in between in
// as few launches as the per-item workspace allows (`bulk` items each) on a second, HIGH-PRIORITY compute stream when the
// kernel family can run on two (`two_streams`): the first stage's kernel covers the upload of the rest, the bulk takes the SIMDs
// over as soon as it has arrived, and the last stage -- queued BEHIND the first on the normal-priority stream -- only fills what
// the bulk's tail leaves idle and is still computing while the bulk's results go down.  (Round 3 first used equal stages: 8
// boundaries for 65 536 items, 94-96 % of the resident rate.)  Stages on different streams get disjoint ranges
// [ws_offset, ws_offset + nb) of the `ws_total` workspace slots.
struct PgdbStage { int64_t b0, nb; bool second; int64_t ws_offset; };
struct PgdbStagePlan { std::vector<PgdbStage> stages; int64_t ws_total = 0; };

inline PgdbStagePlan pgdb_stage_plan(int64_t B, int64_t host_chunk, bool two_streams, int64_t bulk = 65536) {
    PgdbStagePlan p;
    const int64_t first = host_chunk < B / 2 ? host_chunk : B / 2;
    const int64_t last = (B >= 4 * host_chunk) ? host_chunk : 0;
    p.stages.push_back({0, first, false, 0});
    for (int64_t b0 = first; b0 < B - last; b0 += bulk)
        p.stages.push_back({b0, (B - last - b0 < bulk ? B - last - b0 : bulk), two_streams, two_streams ? first : 0});
    if (last) p.stages.push_back({B - last, last, false, 0});
    const int64_t mid_slots = (B - last - first) < bulk ? (B - last - first) : bulk;
    p.ws_total = two_streams ? first + mid_slots : (first > mid_slots ? first : mid_slots);
    return p;
}

}  // namespace fbx
