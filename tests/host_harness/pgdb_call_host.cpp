// Host build of csrc/fbx_pgdb_call.hpp for tests/test_pgdb_call_host.py (test infrastructure only -- the package never loads it):
// the call record's slice() and the stage plan of the pipelined host-pointer entry point, through a flat C interface.
#include "../../forest-benchmarking_amd/csrc/fbx_pgdb_call.hpp"

using fbx::PgdbCall;

namespace {
// the record as 21 integers (pointers as addresses) in the order of FIELDS in the test, eig_rel_tol beside them
enum { DES, B_, E, C, TP, MODE, MAX_ITERS, CHOI, IT, DY, BT, COST, SW, TRACE, TRACE_ITERS, LAUNCH_STREAM, WS_ITEMS, WS_OFFSET,
       TOTAL_BATCH, M, DD, NFIELDS };

template <class T> T* ptr(int64_t v) { return reinterpret_cast<T*>(static_cast<intptr_t>(v)); }
template <class T> int64_t addr(T* p) { return static_cast<int64_t>(reinterpret_cast<intptr_t>(p)); }

PgdbCall unpack(const int64_t* f, double tol) {
    PgdbCall c;
    c.des = ptr<const fbx_design>(f[DES]); c.B = f[B_]; c.e = ptr<const double>(f[E]); c.c = ptr<const double>(f[C]);
    c.tp = (int)f[TP]; c.mode = (int)f[MODE]; c.max_iters = (int)f[MAX_ITERS];
    c.choi = ptr<double>(f[CHOI]); c.it = ptr<int32_t>(f[IT]); c.dy = ptr<int32_t>(f[DY]); c.bt = ptr<int32_t>(f[BT]);
    c.cost = ptr<double>(f[COST]); c.sw = ptr<int32_t>(f[SW]); c.eig_rel_tol = tol; c.trace = ptr<int32_t>(f[TRACE]);
    c.trace_iters = (int)f[TRACE_ITERS]; c.launch_stream = ptr<ihipStream_t>(f[LAUNCH_STREAM]);
    c.ws_items = f[WS_ITEMS]; c.ws_offset = f[WS_OFFSET]; c.total_batch = f[TOTAL_BATCH];
    c.m = (size_t)f[M]; c.DD = (size_t)f[DD];
    return c;
}
void pack(const PgdbCall& c, int64_t* f, double* tol) {
    f[DES] = addr(c.des); f[B_] = c.B; f[E] = addr(c.e); f[C] = addr(c.c); f[TP] = c.tp; f[MODE] = c.mode; f[MAX_ITERS] = c.max_iters;
    f[CHOI] = addr(c.choi); f[IT] = addr(c.it); f[DY] = addr(c.dy); f[BT] = addr(c.bt); f[COST] = addr(c.cost); f[SW] = addr(c.sw);
    f[TRACE] = addr(c.trace); f[TRACE_ITERS] = c.trace_iters; f[LAUNCH_STREAM] = addr(c.launch_stream);
    f[WS_ITEMS] = c.ws_items; f[WS_OFFSET] = c.ws_offset; f[TOTAL_BATCH] = c.total_batch; f[M] = (int64_t)c.m; f[DD] = (int64_t)c.DD;
    *tol = c.eig_rel_tol;
}
}  // namespace

extern "C" {

int pgdb_call_host_nfields() { return NFIELDS; }

// `n` slices applied one after the other: cuts[2 k], cuts[2 k + 1] = b0, nb of slice k
void pgdb_call_host_slice(const int64_t* in, double tol_in, int n, const int64_t* cuts, int64_t* out, double* tol_out) {
    PgdbCall c = unpack(in, tol_in);
    for (int k = 0; k < n; ++k) c = c.slice(cuts[2 * k], cuts[2 * k + 1]);
    pack(c, out, tol_out);
}

// stages as (b0, nb, second, ws_offset) rows; returns their number (only the first `cap` are written)
int pgdb_call_host_plan(int64_t B, int64_t host_chunk, int two_streams, int64_t bulk, int64_t* stages, int cap, int64_t* ws_total) {
    const fbx::PgdbStagePlan p = bulk > 0 ? fbx::pgdb_stage_plan(B, host_chunk, two_streams != 0, bulk)
                                          : fbx::pgdb_stage_plan(B, host_chunk, two_streams != 0);      // the product's bulk size
    for (int k = 0; k < (int)p.stages.size() && k < cap; ++k) {
        stages[4 * k] = p.stages[k].b0; stages[4 * k + 1] = p.stages[k].nb;
        stages[4 * k + 2] = p.stages[k].second ? 1 : 0; stages[4 * k + 3] = p.stages[k].ws_offset;
    }
    *ws_total = p.ws_total;
    return (int)p.stages.size();
}

}  // extern "C"
