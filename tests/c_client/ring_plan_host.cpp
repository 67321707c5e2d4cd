// The ring streams' window arithmetic and block counting (pyitd_amd/csrc/itd_ring_plan.hpp) built for the host, behind a few
// accessors for tests/test_ring_plan_host.py.  g++ -O2 -std=c++17 -Wall -Werror -fPIC -shared; no HIP.
#include "../../pyitd_amd/csrc/itd_ring_plan.hpp"

using namespace itd;

namespace {
// what ring_step of itd_ring_streams.inc does with a step, less the launch: plan it on the count as the step sees it
struct Planner {
    const RingCount *c;
    int64_t L, D, H, reach;
    bool stores;
    int fail;                      // what the launch reports
    int64_t *b_out;
    int32_t *fields;               // emit, store_slot, slot0, rd_lo, rd_hi, at_start, at_end
    int64_t *wide;                 // base, arr
    int operator()(int64_t b) const
    {
        RingStepArgs a = {};
        ring_plan(a, c->t, c->P, L, D, H, reach, b, stores);
        *b_out = b;
        const int32_t f[7] = {a.emit, a.store_slot, a.slot0, a.rd_lo, a.rd_hi, a.at_start, a.at_end};
        for (int i = 0; i < 7; ++i) fields[i] = f[i];
        wide[0] = a.base;
        wide[1] = a.arr;
        return fail;
    }
};
}  // namespace

extern "C" {

int ring_args_bytes() { return (int)sizeof(RingStepArgs); }

void ring_count_fresh(int64_t *c) { const RingCount f = kRingCountFresh; c[0] = f.t; c[1] = f.P; c[2] = f.sent; }
int64_t ring_count_held(const int64_t *c) { return ring_held(RingCount{c[0], c[1], c[2]}); }
int ring_count_flushing(const int64_t *c) { return ring_flushing(RingCount{c[0], c[1], c[2]}) ? 1 : 0; }

// One push (flush = 0) or flush step (flush = 1) on the count c = (t, P, sent), whose launch reports `fail`.  ran: the step was
// planned; then b, fields and wide hold its plan.  Returns what ring_push / ring_flush return.
int ring_count_step(int64_t *c, int64_t L, int64_t D, int64_t H, int64_t reach, int flush, int fail, int32_t *emitted, int32_t *ran,
                    int64_t *b, int32_t *fields, int64_t *wide)
{
    RingCount rc = {c[0], c[1], c[2]};
    *b = INT64_MIN;
    const Planner step = {&rc, L, D, H, reach, !flush, fail, b, fields, wide};
    const int r = flush ? ring_flush(rc, emitted, step) : ring_push(rc, D, emitted, step);
    *ran = *b != INT64_MIN;
    c[0] = rc.t; c[1] = rc.P; c[2] = rc.sent;
    return r;
}

}  // extern "C"
