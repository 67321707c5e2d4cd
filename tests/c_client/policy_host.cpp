// Host build of pyitd_amd/csrc/itd_policy.hpp for tests/test_policy_host.py: the engine's choice of form and what it learns when a
// form falls short, driven call by call without a GPU, and the spline operators' form.  Test infrastructure: nothing in pyitd_amd/
// uses this.
#include <string.h>
#include "../../pyitd_amd/csrc/itd_policy.hpp"

extern "C" {
void *policy_new() { return new FormPolicy(); }
void policy_free(void *p) { delete static_cast<FormPolicy *>(p); }

// the setters, by the name of what they set; returns 0, or -1 for an unknown name
int policy_set(void *p, const char *what, int64_t v)
{
    FormPolicy &f = *static_cast<FormPolicy *>(p);
    if (!strcmp(what, "resident_mode")) f.set_resident_mode((int32_t)v);
    else if (!strcmp(what, "l0_mode")) f.set_level0_mode((int32_t)v);
    else if (!strcmp(what, "fuse_mode")) f.set_fuse_mode((int32_t)v);
    else if (!strcmp(what, "fuse_level")) f.set_fuse_level((int32_t)v);
    else if (!strcmp(what, "fuse_range")) f.set_fuse_range((int32_t)v);
    else if (!strcmp(what, "fuse_cap")) f.set_fuse_cap((int32_t)v);
    else if (!strcmp(what, "fuse_min_samples")) f.set_fuse_min_samples(v);
    else return -1;
    return 0;
}

// a field, by name; sets *ok = 0 for an unknown name
int64_t policy_get(const void *p, const char *what, int *ok)
{
    const FormPolicy &f = *static_cast<const FormPolicy *>(p);
    *ok = 1;
#define FIELD(x) if (!strcmp(what, #x)) return (int64_t)f.x;
    FIELD(resident_mode) FIELD(l0_mode) FIELD(fuse_mode) FIELD(fuse_level) FIELD(fuse_range) FIELD(fuse_cap) FIELD(fuse_min_samples)
    FIELD(resident_off_left) FIELD(l0_records_left) FIELD(fuse_off_left) FIELD(fuse_off_span) FIELD(fuse_probe) FIELD(fuse_cap_auto)
    FIELD(fuse_cap_calls) FIELD(fuse_cap_span) FIELD(kf_force_tickets) FIELD(fuse_level2_off) FIELD(kf_shrink) FIELD(fuse_no_memory)
    FIELD(resident_repeats) FIELD(fuse_repeats) FIELD(fuse_signal_repairs) FIELD(device_repairs)
#undef FIELD
    *ok = 0;
    return 0;
}

int policy_resident(void *p, int fits, int timing) { return static_cast<FormPolicy *>(p)->resident(fits != 0, timing != 0); }
int policy_level0_fused(void *p) { return static_cast<FormPolicy *>(p)->level0_fused(); }
int policy_fused_levels(void *p, int64_t n, int64_t seq, int M, int fuse0) { return static_cast<FormPolicy *>(p)->fused_levels(n, seq, M, fuse0 != 0); }
int policy_first_level(const void *p, int64_t seq, int M) { return static_cast<const FormPolicy *>(p)->first_level(seq, M); }
int policy_tiles_per_wg(const void *p) { return static_cast<const FormPolicy *>(p)->tiles_per_wg(); }
int policy_cap(const void *p, int L0, int M) { return static_cast<const FormPolicy *>(p)->cap(L0, M); }
int policy_tickets(const void *p, int64_t wgs, int64_t resident_wgs) { return static_cast<const FormPolicy *>(p)->tickets(wgs, resident_wgs); }

int policy_workspace_unavailable(void *p) { return static_cast<FormPolicy *>(p)->workspace_unavailable(); }
int policy_resident_failed(void *p) { return static_cast<FormPolicy *>(p)->resident_failed(); }
int policy_level0_fell_short(void *p) { return static_cast<FormPolicy *>(p)->level0_fell_short(); }
void policy_fused_levels_delivered(void *p, int capped, int M) { static_cast<FormPolicy *>(p)->fused_levels_delivered(capped != 0, M); }
// 0: fail, 1: repair the failed signals, 2: repeat the call
int policy_fused_levels_refused(void *p, int bits, int fail_lev, int L0, int cap, int M, int nfail, int batch)
{
    return (int)static_cast<FormPolicy *>(p)->fused_levels_refused(bits, fail_lev, L0, cap, M, FormPolicy::many(nfail, batch));
}
void policy_device_repaired(void *p, int fixed, int why, int batch, int L0)
{
    static_cast<FormPolicy *>(p)->device_repaired(fixed, why, FormPolicy::many(fixed, batch), L0);
}

// the form a spline extraction takes (0: serial, 1: parallel in the knots, 2: one workgroup) and whether MEITD's loop is one launch
int policy_spline_form(int solver, int64_t n, int batch)
{
    const SplineForm f = spline_form(solver, n, batch);
    return f == SplineForm::Serial ? 0 : f == SplineForm::Parallel ? 1 : 2;
}
int policy_meitd_one_launch(int solver, int64_t n) { return meitd_one_launch(solver, n); }
}
