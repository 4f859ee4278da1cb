// lqmpc_api.hip -- host side of the C ABI declared in include/lqmpc.h: handle, argument checks,
// shared-block packing, workspace management, kernel dispatch, host<->device staging.
#include "lqmpc_launch.h"
#include "lqmpc_host.h"
#include "../../include/lqmpc.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using lqmpc::KParams;

static thread_local std::string g_err;

static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(LQMPC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct HostBuf {                     // pinned host memory (hipHostMalloc) + the event of the last copy that read / wrote it
    void *p = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool ev_valid = false;
};

struct lqmpc_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    lqmpc_options opt;
    DevBuf shared, ws;
    DevBuf key, perm, rec;           // difficulty ordering of rollout batches (its counters live in `fail`)
    DevBuf fail;                     // [count (2) | counters of the difficulty order | list] of the instances handed to the packed kernel
    bool fail_cleared = false;       // build_order zeroed count and counters in this call already
    bool hist_ready = false;         // both sets of order counters are zero / being zeroed by the probe launches: no fill needed
    int hist_turn = 0;               // which set the next probe counts into
    DevBuf st2, it2;                 // lqmpc_sweep_batch_dev without a fused kernel: status / iters of the max-V_N pass
    DevBuf sens_u, sens_x, sens_st;  // lqmpc_*_sens*: the plan, its states and the status where the caller passed NULL
    DevBuf cgrad_part;               // lqmpc_*_cost_grad* with reduce: the partial sums of every wavefront
    DevBuf rcgrad_part;              // lqmpc_rollout_cost_grad_batch* with reduce: the partial sums of every wavefront
    DevBuf tape;                     // lqmpc_rollout_tape_batch_dev: x_t of two steps in turn, u_0, V_N, status and iters of one solve
    DevBuf arena;                    // host-flavour staging (Stager): every array of the call in one block
    HostBuf arena_pin;               // ... its pinned image, for the small calls that go up and come back in one copy each
    HostBuf shared_pin[2];           // source of the shared block's upload
    int shared_turn = 0;
    std::vector<double> shared_host; // last uploaded shared block
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string last_kernel = "none";
    uint64_t last_owner = 0;         // the id of the controller whose record path set last_kernel; 0: a one-shot call did
    uint64_t ctl_ids = 0;            // ids given to controllers so far
};

constexpr int JIT_FALLBACK_COLS = 1024;   // workspace columns of the generic kernel when it only serves a hand-back list

constexpr size_t HIST_INTS = (size_t)lqmpc::ORDER_BUCKETS * lqmpc::ORDER_PAD;
constexpr size_t FAIL_HDR = 16 + 2 * HIST_INTS;    // ints in front of the hand-back list: its count, the order's two alternating sets of counters

static int ensure_host(HostBuf &b, size_t bytes)
{
    if (!b.ev) {
        hipError_t e = hipEventCreateWithFlags(&b.ev, hipEventDisableTiming);
        if (e != hipSuccess) { b.ev = nullptr; return fail(LQMPC_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e)); }
    }
    if (bytes <= b.cap) return 0;
    if (b.p) {
        if (b.ev_valid) (void)hipEventSynchronize(b.ev);
        (void)hipHostFree(b.p);
        b.p = nullptr; b.cap = 0; b.ev_valid = false;
    }
    const size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
    if (e != hipSuccess) { b.p = nullptr; return fail(LQMPC_ERR_ALLOC, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
    b.cap = want;
    return 0;
}

static int ensure(lqmpc_handle *h, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return 0;
    if (b.p) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipFree(b.p));
        b.p = nullptr; b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) { b.p = nullptr; return fail(LQMPC_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    b.cap = want;
    return 0;
}

// The buffer that holds the hand-back count, the order's counters and the hand-back list.  A re-allocated buffer holds undefined
// counters (hipMalloc may even hand the old address back), so the no-fill path of build_order is switched off by CAPACITY.
static int ensure_fail(lqmpc_handle *h, size_t bytes)
{
    const size_t cap_before = h->fail.cap;
    const int rc = ensure(h, h->fail, bytes);
    if (h->fail.cap != cap_before || rc) h->hist_ready = false;
    return rc;
}

extern "C" {

const char *lqmpc_version(void) { return "lqmpc-mi355x 0.2.0 (gfx950, fp64)"; }
const char *lqmpc_last_error(void) { return g_err.c_str(); }

int lqmpc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void lqmpc_default_options(lqmpc_options *opt)
{
    if (!opt) return;
    opt->struct_size = (uint32_t)sizeof(lqmpc_options);
    opt->reserved = 0;
    opt->eps = 1e-12;
    opt->tau = 0.999;
    opt->z0_scale = 0.1;
    opt->max_iter = 50;
    opt->polish = 1;
    opt->kernel = LQMPC_KERNEL_AUTO;
    opt->presolve = -1;
    opt->order = -1;
    opt->warm_start = -1;
    opt->layout = -1;
    opt->r16_maxit = 12;
    opt->r16_build = -1;
    opt->nwide = -1;
    opt->jit = -1;
    opt->ctl_wg = 0;
}

int lqmpc_create_on_stream(int device, void *hip_stream, lqmpc_handle **out)
{
    if (!out) return fail(LQMPC_ERR_BAD_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(LQMPC_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(LQMPC_ERR_BAD_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    lqmpc_handle *h = new lqmpc_handle();
    h->device = device;
    h->stream = (hipStream_t)hip_stream;
    h->own_stream = false;
    lqmpc_default_options(&h->opt);
    hipError_t e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    if (e != hipSuccess) { delete h; return fail(LQMPC_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e)); }
    *out = h;
    return 0;
}

int lqmpc_create(int device, lqmpc_handle **out)
{
    int rc = lqmpc_create_on_stream(device, nullptr, out);
    if (rc) return rc;
    hipStream_t s;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) { lqmpc_destroy(*out); *out = nullptr; return fail(LQMPC_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    (*out)->stream = s;
    (*out)->own_stream = true;
    return 0;
}

int lqmpc_destroy(lqmpc_handle *h)
{
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (DevBuf *b : {&h->shared, &h->ws, &h->key, &h->perm, &h->rec, &h->fail, &h->st2, &h->it2, &h->sens_u, &h->sens_x, &h->sens_st, &h->cgrad_part, &h->rcgrad_part, &h->tape, &h->arena}) if (b->p) (void)hipFree(b->p);
    for (HostBuf *b : {&h->arena_pin, &h->shared_pin[0], &h->shared_pin[1]}) {
        if (b->p) (void)hipHostFree(b->p);
        if (b->ev) (void)hipEventDestroy(b->ev);
    }
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

int lqmpc_sync(lqmpc_handle *h)
{
    if (!h) return fail(LQMPC_ERR_BAD_ARG, "handle is NULL");
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int lqmpc_set_options(lqmpc_handle *h, const lqmpc_options *opt)
{
    if (!h || !opt) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (opt->struct_size != sizeof(lqmpc_options))
        return fail(LQMPC_ERR_BAD_ARG, "lqmpc_options.struct_size does not match this library: built against another lqmpc.h? "
                                       "(start from lqmpc_default_options / lqmpc_get_options)");
    if (!(opt->eps > 0.0 && opt->eps < 1.0)) return fail(LQMPC_ERR_BAD_ARG, "eps must be in (0,1)");
    if (!(opt->tau > 0.0 && opt->tau < 1.0)) return fail(LQMPC_ERR_BAD_ARG, "tau must be in (0,1)");
    if (!(opt->z0_scale > 0.0)) return fail(LQMPC_ERR_BAD_ARG, "z0_scale must be positive");
    if (opt->max_iter < 1 || opt->max_iter > 1000) return fail(LQMPC_ERR_BAD_ARG, "max_iter must be in [1,1000]");
    if (opt->kernel < LQMPC_KERNEL_AUTO || opt->kernel > LQMPC_KERNEL_WORKGROUP) return fail(LQMPC_ERR_BAD_ARG, "unknown kernel selector");
    if (opt->presolve < -1 || opt->presolve > 1) return fail(LQMPC_ERR_BAD_ARG, "presolve must be -1, 0 or 1");
    if (opt->order < -1 || opt->order > 1) return fail(LQMPC_ERR_BAD_ARG, "order must be -1, 0 or 1");
    if (opt->warm_start < -1 || opt->warm_start > 1) return fail(LQMPC_ERR_BAD_ARG, "warm_start must be -1, 0 or 1");
    if (opt->layout < -1 || opt->layout > 1) return fail(LQMPC_ERR_BAD_ARG, "layout must be -1, 0 or 1");
    if (opt->r16_maxit < 0 || opt->r16_maxit > 64) return fail(LQMPC_ERR_BAD_ARG, "r16_maxit must be in [0,64]");
    if (opt->r16_build < -1 || opt->r16_build > 1) return fail(LQMPC_ERR_BAD_ARG, "r16_build must be -1, 0 or 1");
    if (opt->nwide < -1) return fail(LQMPC_ERR_BAD_ARG, "nwide must be -1 (auto) or a count");
    if (opt->jit < -1 || opt->jit > 2) return fail(LQMPC_ERR_BAD_ARG, "jit must be -1, 0, 1 or 2");
    if (opt->ctl_wg < 0 || opt->ctl_wg > 1) return fail(LQMPC_ERR_BAD_ARG, "ctl_wg must be 0 or 1");
    h->opt = *opt;
    return 0;
}

int lqmpc_get_options(const lqmpc_handle *h, lqmpc_options *opt)
{
    if (!h || !opt) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    *opt = h->opt;
    return 0;
}

int lqmpc_has_specialization(int nx, int nu, int N) { return lqmpc::spec_available(nx, nu, N) ? 1 : 0; }

const char *lqmpc_last_kernel(const lqmpc_handle *h) { return h ? h->last_kernel.c_str() : "none"; }

}  // extern "C"

// ------------------------------------------------------------------------------------------
static int check_dims(int nx, int nu, int N, int64_t Bsz)
{
    if (nx < 1 || nu < 1 || N < 1 || Bsz < 1) return fail(LQMPC_ERR_BAD_ARG, "nx, nu, N and Bsz must be positive");
    if (nx > LQMPC_MAX_NX || nu > LQMPC_MAX_NU || N > LQMPC_MAX_N || N * nu > LQMPC_MAX_NVAR) {
        char buf[160];
        snprintf(buf, sizeof buf, "dims over the build limits (nx<=%d, nu<=%d, N<=%d, N*nu<=%d)", LQMPC_MAX_NX, LQMPC_MAX_NU,
                 LQMPC_MAX_N, LQMPC_MAX_NVAR);
        return fail(LQMPC_ERR_BAD_ARG, buf);
    }
    return 0;
}

struct Call {
    int nx, nu, N, T, K, mode, true_per_instance;
    int64_t Bsz;
    const double *Q, *R, *P, *lb, *ub, *x_ref, *u_ref, *At_sh, *Bt_sh, *x0s;
};

// references or an off-centre box: the linear term has a constant part (lqmpc_reserve plans without a box)
static bool has_lin(const Call &c)
{
    bool lin = c.x_ref || c.u_ref;
    for (int k = 0; c.lb && c.ub && k < c.nu; ++k) lin = lin || (c.ub[k] + c.lb[k] != 0.0);
    return lin;
}

// Everything the host decides about one call before it enqueues anything (make_plan); the entry points, build_order, launch, the
// hand-back pass and lqmpc_reserve only read it.
enum Family {
    FAM_GENERIC,         // lqmpc_generic.hip, workspace in HBM
    FAM_WG,              // lqmpc_wg.hip, one instance per workgroup
    FAM_SPEC,            // lqmpc_spec.hip, packed register-resident
    FAM_SPEC_TIERED,     // ... a sorted rollout whose first nwide slots get the 16-lane-row layout, then the packed kernel over its hand-back list
    FAM_R16,             // lqmpc_r16.hip, prebuilt 16-lane-row kernel on the whole batch, then the packed kernel over its hand-back list
    FAM_JIT,             // lqmpc_jit.hip, run-time compiled 16-lane-row kernel, then the generic kernel over its hand-back list
};
struct Plan {
    Family family;
    bool order;          // build the difficulty order (probe + scatter) in front of the first pass
    bool order_roll;     // the host computes the first gain for the order's key (KParams::order_roll)
    long long nwide;     // FAM_SPEC_TIERED: slots of the wide tier
    long long ws_cols;   // workspace columns of the generic kernel; 0: the call needs no workspace
    int presolve, warm_start;   // options.presolve / warm_start with their defaults resolved
    bool has_lin;        // has_lin() of the call
    // the 16-lane-row kernels on the whole batch: every mode, the sweep fused into one launch (otherwise it is the two-launch fall-back)
    bool rows() const { return family == FAM_R16 || family == FAM_JIT; }
    // the hand-back list goes to the generic kernel over a list, with ws_cols columns (otherwise to the packed kernel)
    bool list_generic() const { return family == FAM_JIT; }
};

// The routing of one call: a function of the options, the call and the device, nothing else.  The only refusals are a forced kernel
// that does not serve the shape; a failed run-time compile is not one (lqmpc_last_error says why, the call falls to the next family).
static int make_plan(const lqmpc_options &o, const Call &c, int device, Plan &pl)
{
    const int nx = c.nx, nu = c.nu, N = c.N;
    const int presolve = pl.presolve = o.presolve < 0 ? 1 : o.presolve;
    const int warm_start = pl.warm_start = o.warm_start < 0 ? presolve : o.warm_start;
    pl.has_lin = has_lin(c);
    const bool built = lqmpc::spec_available(nx, nu, N);
    if (o.kernel == LQMPC_KERNEL_SPECIALIZED && !built)
        return fail(LQMPC_ERR_UNSUPPORTED, "no register-resident specialisation built for these dims");
    const bool spec = built && o.kernel != LQMPC_KERNEL_GENERIC && o.kernel != LQMPC_KERNEL_WORKGROUP;
    // a shape without a prebuilt instantiation inside the 16-lane-row domain: compile its kernel now (first use: ~2 s; then cached).
    // The algorithm is the presolve + warm-started active set, so the option combinations that switch those off stay on the
    // generic / workgroup kernels, as do the shapes whose compile fails (no hiprtc on the machine: reported by last_error once).
    bool jit = false;
    if (o.kernel == LQMPC_KERNEL_AUTO && o.jit != 0 && !built && presolve && warm_start && c.Bsz <= INT32_MAX &&
        lqmpc::jit_r16_shape(nx, nu, N, nullptr, o.jit == 2)) {
        std::string why;
        jit = lqmpc::jit_available(device, nx, nu, N, c.mode, &why, o.jit == 2);
        if (!jit) g_err = "run-time compile unavailable, using the generic kernels: " + why;
    }
    const bool wg = !spec && !jit && (o.kernel == LQMPC_KERNEL_AUTO || o.kernel == LQMPC_KERNEL_WORKGROUP) && lqmpc::wg_supported(nx, nu, N);
    if (o.kernel == LQMPC_KERNEL_WORKGROUP && !wg)
        return fail(LQMPC_ERR_UNSUPPORTED, "the workgroup kernel needs 32 < N*nu <= 128, nx <= 16, nu <= 8 and an LDS image within 160 KiB");
    // Which layout where a shape has both specialisations (measured at C3 / C2 shapes).  Rollouts: the
    // 16-lane-row kernel (two waves per SIMD, P and W packed in LDS) for every batch size -- 0.77 ms against 0.97 ms for the two-tier
    // launch of the packed kernel at C3's 65 536 instances, and it also fills the GPU where the packed kernel (16 or 32 instances
    // per wavefront) cannot.  One-shot entry points and the fused sweep (built for one wave per SIMD): up to `limit` instances
    // (max V_N with n <= 10 and a large batch: the packed kernel's one lane per instance wins the K-state loop, 0.24 against 0.36 ms
    // at C2 x 65 536).  options.layout = 0/1 forces the choice (0 gives the packed kernel and its two-tier launch).
    const int64_t limit = (c.mode == lqmpc::MODE_MAXVN && N * nu <= 10) ? 32768 : INT32_MAX;
    bool r16 = spec && o.kernel == LQMPC_KERNEL_AUTO && presolve && warm_start && lqmpc::r16_available(nx, nu, N) && c.Bsz <= INT32_MAX;
    if (r16 && lqmpc::r16_lanes(nx, nu, N) == 64) r16 = o.layout != 0;   // vs one wave per instance in the packed family too: always
    else r16 = r16 && (o.layout >= 0 ? o.layout == 1 : c.Bsz <= limit);
    pl.family = jit ? FAM_JIT : r16 ? FAM_R16 : spec ? FAM_SPEC : wg ? FAM_WG : FAM_GENERIC;

    // The difficulty order of a rollout (options.order; the two-launch sweep leaves it to the rollout it calls).  The packed family
    // orders from 1 024 instances; the 16-lane-row family from 8 192 (measured at C3: the sorted walk pays for its probe and scatter
    // launches from about 8 192 instances: 0.26 against 0.31 ms at 16 384, 0.25 against 0.19 ms at 4 096).
    // Measured again with the cheaper probe and scatter (C3, T = 30, order on against off): 0.176 against 0.150 ms at 4 096, 0.191 against
    // 0.179 ms at 8 192, 0.195 against 0.215 ms at 16 384.  The crossing still lies between 8 192 and 16 384; the threshold stays.
    // And with no records staged under the roll key: 0.177 against 0.150 ms at 4 096, 0.190 against 0.180 ms at 8 192, 0.192 against
    // 0.217 ms at 16 384 (profiles/order_split_speed.json): the same.
    const bool rollout = c.mode == lqmpc::MODE_ROLLOUT || c.mode == lqmpc::MODE_SWEEP;
    const bool packed_size = c.T >= 4 && c.Bsz >= 1024;
    if (pl.rows()) pl.order = rollout && (o.order < 0 ? (c.T >= 4 && c.Bsz >= 8192) : o.order == 1);
    else pl.order = c.mode == lqmpc::MODE_ROLLOUT && spec && (o.order < 0 ? (presolve && packed_size) : o.order == 1);
    // The order's key for rollouts on a shared plant with zero references and a centred box (lqmpc_probe.h): a clipped roll of the
    // PLANT under the first gain of the N-stage problem on it -- the closed loop every instance of the batch runs in.  Only where an
    // order can be built at all (the looser of the two sizes): small batches skip the host's Riccati steps.
    const bool may_order = o.order > 0 || (o.order < 0 && packed_size);
    pl.order_roll = may_order && rollout && nu <= 8 && !c.true_per_instance && c.At_sh && c.Bt_sh && !pl.has_lin;
    // the hardest instances (first in the order) in the 16-lane-row layout: see lqmpc_spec_tiered_kernel
    pl.nwide = 0;
    if (pl.order && pl.family == FAM_SPEC && lqmpc::spec_tiered_available(nx, nu, N) && presolve && warm_start && c.Bsz <= INT32_MAX) {
        const long long nw = o.nwide >= 0 ? o.nwide : (c.Bsz / 8 < 4096 ? c.Bsz / 8 : 4096) / 4 * 4;   // measured: ~one 16-lane-row wave per SIMD
        pl.nwide = nw < 0 ? 0 : (nw > c.Bsz ? c.Bsz : nw);
        if (pl.nwide > 0) pl.family = FAM_SPEC_TIERED;
    }
    // Generic workspace: a column per instance of the batch (in whole wavefronts) where the generic kernel runs the call; behind a
    // run-time compiled kernel it only ever sees the instances that kernel hands back -- a bounded workspace, walked by a
    // grid-stride loop
    pl.ws_cols = pl.family == FAM_JIT ? JIT_FALLBACK_COLS : pl.family == FAM_GENERIC ? (c.Bsz + 63) / 64 * 64 : 0;
    return 0;
}

static int ensure_ws(lqmpc_handle *h, const Call &c, const Plan &pl)
{
    return ensure(h, h->ws, (size_t)lqmpc::generic_ws_entries(c.nx, c.nu, c.N) * (size_t)pl.ws_cols * sizeof(double));
}

// key, permutation, counters (in front of the hand-back list) and, where the call stages them (`records`: build_order), the
// instance-major records of a difficulty order over B instances
static int ensure_order(lqmpc_handle *h, int nx, int nu, size_t B, bool records)
{
    int rc = ensure(h, h->key, B * sizeof(double));
    if (!rc) rc = ensure(h, h->perm, B * sizeof(int));
    if (!rc) rc = ensure_fail(h, (B + FAIL_HDR) * sizeof(int));
    if (!rc && records) rc = ensure(h, h->rec, B * (size_t)(nx * nx + nx * nu + nx) * sizeof(double));
    return rc;
}

// The checks every call makes of its dimensions, weights and box before anything is enqueued.
static int check_call(const Call &c)
{
    int rc = check_dims(c.nx, c.nu, c.N, c.Bsz);
    if (rc) return rc;
    if (!c.Q || !c.R || !c.P || !c.lb || !c.ub) return fail(LQMPC_ERR_BAD_ARG, "Q, R, P, lb, ub must not be NULL");
    for (int k = 0; k < c.nu; ++k)
        if (!(c.ub[k] > c.lb[k]) || !std::isfinite(c.lb[k]) || !std::isfinite(c.ub[k]))
            return fail(LQMPC_ERR_BAD_ARG, "every input needs a finite box with lb < ub");
    // the kernels shift the box to its centre (u = v + c): a centre far out makes the answer inaccurate (include/lqmpc.h, "Box limit")
    for (int k = 0; k < c.nu; ++k)
        if (!(std::fabs(0.5 * c.lb[k] + 0.5 * c.ub[k]) <= LQMPC_MAX_BOX_CENTRE)) {
            char buf[256];
            snprintf(buf, sizeof buf, "box of input %d is centred at %.17g: |lb + ub| / 2 must be <= %g (LQMPC_MAX_BOX_CENTRE); write a "
                     "one-sided limit with a finite other side near the largest input expected", k, 0.5 * c.lb[k] + 0.5 * c.ub[k],
                     (double)LQMPC_MAX_BOX_CENTRE);
            return fail(LQMPC_ERR_BAD_ARG, buf);
        }
    return 0;
}

static int upload_block(lqmpc_handle *h, std::vector<double> &sh);

// Pack the batch-shared data of a call (Kg: the first gain of an order's roll key, or null = zeros) and upload it, skipped when
// identical to the last upload; `so` takes the offsets.  The block of a post-pass is the block of the solve it follows, bit for bit.
static int upload_shared(lqmpc_handle *h, const Call &c, const double *Kg, lqmpc::SharedOff &so)
{
    const int nx = c.nx, nu = c.nu, N = c.N;
    std::vector<double> sh;
    auto put = [&](const double *src, int count) {
        int off = (int)sh.size();
        sh.resize(sh.size() + count, 0.0);
        if (src) memcpy(sh.data() + off, src, sizeof(double) * count);
        return off;
    };
    so.Q = put(c.Q, nx * nx);
    so.R = put(c.R, nu * nu);
    so.P = put(c.P, nx * nx);
    so.lb = put(c.lb, nu);
    so.ub = put(c.ub, nu);
    so.xref = put(c.x_ref, nx * N);
    so.uref = put(c.u_ref, nu * N);
    so.At = put(c.true_per_instance ? nullptr : c.At_sh, nx * nx);
    so.Bt = put(c.true_per_instance ? nullptr : c.Bt_sh, nx * nu);
    so.x0s = put(c.x0s, c.x0s ? nx * c.K : 1);
    so.Kg = put(Kg, nu * nx);
    return upload_block(h, sh);
}

// The packed shared block of a call on its way to the device, skipped when identical to the last upload.
static int upload_block(lqmpc_handle *h, std::vector<double> &sh)
{
    int rc = ensure(h, h->shared, sh.size() * sizeof(double));
    if (rc) return rc;
    if (sh != h->shared_host) {
        // The device copy may still be read by an earlier launch on this stream: the copy is ordered behind it by the stream.  No
        // host-side wait: the source is pinned memory owned by the handle (two buffers taken in turn, so that the copy of this call
        // cannot be overwritten by the next call's packing while it is still in flight).
        const size_t bytes = sh.size() * sizeof(double);
        HostBuf &hb = h->shared_pin[h->shared_turn ^= 1];
        int rc2 = ensure_host(hb, bytes);
        if (rc2) return rc2;
        if (hb.ev_valid) HIP_TRY(hipEventSynchronize(hb.ev));       // (two calls back: long done, costs nothing)
        memcpy(hb.p, sh.data(), bytes);
        HIP_TRY(hipMemcpyAsync(h->shared.p, hb.p, bytes, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipEventRecord(hb.ev, h->stream));
        hb.ev_valid = true;
        h->shared_host.swap(sh);
    }
    return 0;
}

// Check the arguments, plan the call under `opt`, pack the batch-shared data, upload it (skipped when identical to the last upload),
// size the workspace, fill the kernel parameter block.
static int prepare(lqmpc_handle *h, const lqmpc_options &opt, const Call &c, KParams &p, Plan &pl)
{
    h->fail_cleared = false;
    int rc = check_call(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    rc = make_plan(opt, c, h->device, pl);
    if (rc) return rc;
    const int nx = c.nx, nu = c.nu, N = c.N;
    memset(&p, 0, sizeof p);
    std::vector<double> Kg((size_t)nu * nx, 0.0);
    const bool roll = pl.order_roll && host_first_gain(nx, nu, N, c.At_sh, c.Bt_sh, c.Q, c.R, c.P, Kg.data());
    rc = upload_shared(h, c, roll ? Kg.data() : nullptr, p.so);
    if (rc) return rc;
    p.order_roll = roll ? 1 : 0;
    p.nx = nx; p.nu = nu; p.N = N; p.n = N * nu;
    p.T = c.T; p.K = c.K; p.mode = c.mode;
    p.true_per_instance = c.true_per_instance;
    p.has_ref = (c.x_ref || c.u_ref) ? 1 : 0;
    p.has_lin = pl.has_lin ? 1 : 0;
    p.max_iter = opt.max_iter; p.polish = opt.polish;
    p.presolve = pl.presolve; p.warm_start = pl.warm_start;
    p.eps = opt.eps; p.tau = opt.tau; p.z0_scale = opt.z0_scale;
    p.Bsz = c.Bsz;
    p.sh = (const double *)h->shared.p;
    p.r16_maxit = opt.r16_maxit;                               // a small cap exercises the hand-back path (tests)
    p.r16_build = opt.r16_build;
    if (pl.ws_cols) {
        p.ws_stride = pl.ws_cols;
        rc = ensure_ws(h, c, pl);
        if (rc) return rc;
        p.ws = (double *)h->ws.p;
    }
    return 0;
}

// Difficulty ordering (options.order): probe launch -> (bucket, position) per instance -> scatter, hardest first.
// On success p.perm points at the permutation (slot -> instance).
// The order only has to group similar instances: a bucket sort over the logarithm of the probe's key (lqmpc_probe_kernel),
// two launches instead of the eight of a full radix / merge sort (41 us of a 0.51 ms C3 launch).  Which instance gets which
// position inside a bucket depends on the order of the atomics, i.e. the permutation is not reproducible run to run; the
// results are, because no result depends on the instances that share a wavefront.
static int build_order(lqmpc_handle *h, const Plan &pl, KParams &p)
{
    if (p.Bsz > (long long)INT32_MAX) return fail(LQMPC_ERR_BAD_ARG, "ordering supports up to 2^31-1 instances");
    // No staged records under the roll key for the 16-lane-row kernels with four instances a wavefront (n <= 32): the probe then reads
    // x0 alone and the sorted walk reads the instance-minor arrays through the permutation.  Measured at C3 x 65 536: staging costs
    // the probe 7 us (19.6 against 12.5 us; 17.2 us from workgroups of their own in the same launch) and saves the rollout kernel
    // 1 - 3 us (profiles/order_split_c3_summary.txt).  Everything else stages as before, by policy more than by measurement: the
    // free-response key's probe holds A and B anyway; a kernel that gives an instance a whole wavefront or a single lane fetches a
    // contiguous record in fewer lines, but the C4 difference seen (4.131 against 4.138 ms) is inside the run-to-run spread; and the
    // fused sweep rests on one pair (0.827 ms with records, 0.835 ms without).  None of the three was shown to gain without records.
    const bool records = !(p.order_roll && p.mode == lqmpc::MODE_ROLLOUT && pl.rows() && p.n <= 32);
    int rc = ensure_order(h, p.nx, p.nu, (size_t)p.Bsz, records);
    if (rc) return rc;
    // The hand-back count and the order's counters.  First call (or a new buffer): one fill of everything.  After that the probe
    // launch itself zeroes the count and the set of counters the NEXT call will use (the sets alternate), so a call costs no fill
    // launch (4 us of a 0.39 ms C3 call).  Any failure below leaves hist_ready false: the next call fills again.
    if (!h->hist_ready) {
        HIP_TRY(hipMemsetAsync(h->fail.p, 0, FAIL_HDR * sizeof(int), h->stream));
        h->hist_turn = 0;
    }
    h->hist_ready = false;
    h->fail_cleared = true;
    KParams q = p;
    q.mode = lqmpc::MODE_PROBE;
    q.perm = nullptr;
    q.key = (double *)h->key.p;
    q.hist = (int *)h->fail.p + 16 + (size_t)h->hist_turn * HIST_INTS;
    q.hist_next = (int *)h->fail.p + 16 + (size_t)(h->hist_turn ^ 1) * HIST_INTS;
    q.fail_count = (int *)h->fail.p;
    q.stage = records ? (double *)h->rec.p : nullptr;
    const char *name = nullptr;
    if (pl.family == FAM_JIT) {
        std::string why;
        if (!lqmpc::launch_jit(h->device, q, h->stream, &name, &why)) return fail(LQMPC_ERR_UNSUPPORTED, "probe launch failed: " + why);
    } else if (!lqmpc::launch_spec(q, h->stream, &name)) return fail(LQMPC_ERR_UNSUPPORTED, "probe launch failed");
    lqmpc::launch_order_scatter(q, (int *)h->perm.p, h->stream);
    HIP_TRY(hipGetLastError());
    h->hist_turn ^= 1;
    h->hist_ready = true;
    p.perm = (const int *)h->perm.p;
    p.rec = records ? (const double *)h->rec.p : nullptr;
    return 0;
}

// what lqmpc_last_kernel reports: a copy of the name, and which controller's record path it came from (0: none)
static void set_last_kernel(lqmpc_handle *h, const char *name, uint64_t owner = 0)
{
    h->last_kernel = name;
    h->last_owner = owner;
}

// one launch of the packed, workgroup or generic kernel on the whole batch
static int launch(lqmpc_handle *h, const Plan &pl, const KParams &p)
{
    const char *name = "lqmpc_generic_kernel";
    if (pl.family == FAM_SPEC || pl.family == FAM_SPEC_TIERED) {
        if (!lqmpc::launch_spec(p, h->stream, &name)) return fail(LQMPC_ERR_UNSUPPORTED, "specialisation launch failed");
    } else if (pl.family == FAM_WG) {
        if (!lqmpc::launch_wg(p, h->stream, &name)) return fail(LQMPC_ERR_HIP, "workgroup kernel launch failed");
    } else {
        lqmpc::launch_generic(p, h->stream);
    }
    set_last_kernel(h, name);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the hand-back list of this call: count zeroed (by build_order's fill if it ran), list behind the order's counters
static int prepare_hand_back(lqmpc_handle *h, KParams &p)
{
    int rc = ensure_fail(h, ((size_t)p.Bsz + FAIL_HDR) * sizeof(int));
    if (rc) return rc;
    if (!h->fail_cleared) HIP_TRY(hipMemsetAsync(h->fail.p, 0, 2 * sizeof(int), h->stream));
    h->fail_cleared = false;
    p.fail_count = (int *)h->fail.p;
    p.fail_list = (int *)h->fail.p + FAIL_HDR;
    return 0;
}

// Second pass: the instances the first pass `p` handed back (status 3, device-side list), from scratch, in `mode` -- on the packed
// kernel (interior point + polish) where the shape has one, on the generic kernel otherwise.  vn: where V_N goes when p has none.
static int launch_hand_back(lqmpc_handle *h, const Plan &pl, const KParams &p, int mode, double *vn)
{
    KParams f = p;
    f.mode = mode;
    f.perm = p.fail_list; f.count_dev = p.fail_count; f.fail_list = nullptr; f.fail_count = nullptr; f.nwide = 0;
    if (!f.VN) f.VN = vn;
    if (pl.list_generic()) lqmpc::launch_generic_list(f, (int)pl.ws_cols, h->stream);
    else if (!lqmpc::launch_spec(f, h->stream, nullptr)) return fail(LQMPC_ERR_UNSUPPORTED, "hand-back launch failed");
    HIP_TRY(hipGetLastError());
    return 0;
}

// status / iters of the instances on a device-side list: worse status, summed iterations (grid-stride over the list)
__global__ void lqmpc_merge_listed_kernel(int *st, int *it, const int *st2, const int *it2, const int *list, const int *count)
{
    const int n = *count;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int b = list[i];
        if (st) st[b] = st[b] > st2[b] ? st[b] : st2[b];
        if (it) it[b] += it2[b];
    }
}

// 16-lane-row kernel (prebuilt or run-time compiled) on the whole batch, then the hand-back pass over whatever it listed
static int launch_rows(lqmpc_handle *h, const Plan &pl, KParams &p)
{
    int rc = prepare_hand_back(h, p);
    if (rc) return rc;
    const char *name = nullptr;
    if (pl.family == FAM_JIT) {
        std::string why;
        if (!lqmpc::launch_jit(h->device, p, h->stream, &name, &why)) return fail(LQMPC_ERR_HIP, "run-time compiled kernel: " + why);
    } else if (!lqmpc::launch_r16(p, h->stream, &name)) return fail(LQMPC_ERR_UNSUPPORTED, "r16 launch failed");
    HIP_TRY(hipGetLastError());
    const bool sweep = p.mode == lqmpc::MODE_SWEEP;
    if (sweep) {                               // neither second-pass kernel has a fused mode: max V_N, then the rollout, over the list
        // the two passes write status / iters of the listed instances: the max-V_N pass into side buffers, merged below
        // (status = the worse of the two parts, iters = their sum -- the contract of lqmpc_sweep_batch, as on the two-launch path)
        if (p.status) { rc = ensure(h, h->st2, (size_t)p.Bsz * sizeof(int32_t)); if (rc) return rc; }
        if (p.iters) { rc = ensure(h, h->it2, (size_t)p.Bsz * sizeof(int32_t)); if (rc) return rc; }
        KParams m = p;
        m.status = p.status ? (int *)h->st2.p : nullptr;
        m.iters = p.iters ? (int *)h->it2.p : nullptr;
        rc = launch_hand_back(h, pl, m, lqmpc::MODE_MAXVN, nullptr);
        if (rc) return rc;
    }
    rc = launch_hand_back(h, pl, p, sweep ? (int)lqmpc::MODE_ROLLOUT : p.mode, nullptr);
    if (rc) return rc;
    if (sweep && (p.status || p.iters)) {
        const unsigned blocks = (unsigned)(p.Bsz < 65536 ? (p.Bsz + 255) / 256 : 256);
        hipLaunchKernelGGL(lqmpc_merge_listed_kernel, dim3(blocks), dim3(256), 0, h->stream, p.status, p.iters,
                           (const int *)h->st2.p, (const int *)h->it2.p, (const int *)p.fail_list, (const int *)p.fail_count);
        HIP_TRY(hipGetLastError());
    }
    set_last_kernel(h, name);
    return 0;
}

__global__ void lqmpc_merge_status_kernel(int *st, int *it, const int *st2, const int *it2, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (st) st[i] = st[i] > st2[i] ? st[i] : st2[i];
    if (it) it[i] += it2[i];
}

// Every launch of a planned one-shot call whose parameter block is filled: the difficulty order where planned, then the 16-lane-row
// family with its hand-back pass, the two tiers of a sorted packed rollout, or the one launch of the packed, workgroup or generic kernel.
static int run(lqmpc_handle *h, const Plan &pl, KParams &p)
{
    int rc = pl.order ? build_order(h, pl, p) : 0;
    if (rc) return rc;
    if (pl.rows()) return launch_rows(h, pl, p);
    if (pl.family != FAM_SPEC_TIERED) return launch(h, pl, p);
    p.nwide = pl.nwide;
    rc = prepare_hand_back(h, p);
    if (!rc) rc = launch(h, pl, p);
    // second pass: whatever the wide tier handed back (status 3), packed, from the start of the rollout
    return rc ? rc : launch_hand_back(h, pl, p, p.mode, nullptr);
}

// lqmpc_solve_batch_dev under explicit options (a prepared controller passes through here under its own snapshot).  dUplan, dXplan:
// the whole plan of lqmpc_solve_plan_batch_dev (null: none).  The hand-back pass copies the parameter block, so an instance the first
// pass gave up on has its plan rewritten by the second pass, behind the first on the stream.  so: where the call's shared block keeps
// Q, R, P, the box and the references (for the post-pass of the sens calls).
static int solve_dev(lqmpc_handle *h, const lqmpc_options &opt, const Call &c, const double *dA, const double *dB, const double *dx0,
                     double *du0, double *dVN, int32_t *dstatus, int32_t *diters, double *dUplan = nullptr, double *dXplan = nullptr,
                     lqmpc::SharedOff *so = nullptr)
{
    KParams p;
    Plan pl;
    int rc = prepare(h, opt, c, p, pl);
    if (rc) return rc;
    if (so) *so = p.so;
    p.A = dA; p.B = dB; p.x0 = dx0; p.u0 = du0; p.VN = dVN; p.status = dstatus; p.iters = diters;
    p.Uplan = dUplan; p.Xplan = dXplan;
    return run(h, pl, p);
}

// lqmpc_rollout_batch_dev under explicit options (a prepared controller passes through here under its own snapshot)
static int rollout_dev(lqmpc_handle *h, const lqmpc_options &opt, const Call &c, const double *dA, const double *dB, const double *dx0,
                       const double *A_true, const double *B_true, double *dJT, double *dX, double *dU, int32_t *dstatus, int32_t *diters)
{
    KParams p;
    Plan pl;
    int rc = prepare(h, opt, c, p, pl);
    if (rc) return rc;
    p.A = dA; p.B = dB; p.x0 = dx0; p.JT = dJT; p.X = dX; p.U = dU; p.status = dstatus; p.iters = diters;
    if (c.true_per_instance) { p.At = A_true; p.Bt = B_true; }
    return run(h, pl, p);
}

// The sens calls (lqmpc_solve_sens_batch_dev, lqmpc_controller_step_sens_dev): the plan call, then one launch of lqmpc_sens_kernel
// behind it on the stream.  What the post-pass reads of the plan call's outputs and the caller did not ask for (NULL) goes to buffers
// of the handle, grown as needed.
static int sens_buffers(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, double *&dUplan, double *&dXplan, int32_t *&dstatus)
{
    const size_t b = (size_t)Bsz;
    int rc = 0;
    if (!dUplan) { rc = ensure(h, h->sens_u, b * nu * N * sizeof(double)); dUplan = (double *)h->sens_u.p; }
    if (!rc && !dXplan) { rc = ensure(h, h->sens_x, b * nx * (N + 1) * sizeof(double)); dXplan = (double *)h->sens_x.p; }
    if (!rc && !dstatus) { rc = ensure(h, h->sens_st, b * sizeof(int32_t)); dstatus = (int32_t *)h->sens_st.p; }
    return rc;
}

// lqmpc_last_kernel keeps the solve kernel's name
static int sens_launch(lqmpc_handle *h, lqmpc::SensParams &s)
{
    s.sh = (const double *)h->shared.p;
    if (!lqmpc::launch_sens(s, h->stream)) return fail(LQMPC_ERR_HIP, "lqmpc_sens_kernel launch failed");
    HIP_TRY(hipGetLastError());
    return 0;
}

// The model-gradient calls (lqmpc_model_grad_batch_dev, lqmpc_controller_model_grad_dev): the checks, the shared block of `c` (the one
// the plan call before it uploaded, so nothing is copied again) and one launch of lqmpc_grad_kernel.  No solve, no plan: nothing is
// routed or compiled, and lqmpc_last_kernel is left naming the solve kernel.
static int grad_check(const void *owner, const Call *c, const double *Uplan, const double *Xplan, const double *gu0, const double *gVN,
                      const double *gA, const double *gB)
{
    if (!owner || !Uplan || !Xplan || !gA || !gB) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (!gu0 && !gVN) return fail(LQMPC_ERR_BAD_ARG, "gu0 and gVN are both NULL: there is no cotangent");
    if (!c) return 0;                                           // (a controller's own data passed these checks when it was made)
    const int rc = check_call(*c);
    if (rc) return rc;
    if (!lqmpc::grad_fits(c->nx, c->nu, c->N)) {
        char buf[160];
        snprintf(buf, sizeof buf, "lqmpc_grad_kernel needs %zu bytes of LDS at (%d,%d,%d): over 160 KiB", lqmpc::grad_lds_bytes(c->nx, c->nu, c->N),
                 c->nx, c->nu, c->N);
        return fail(LQMPC_ERR_UNSUPPORTED, buf);
    }
    return 0;
}

static int grad_launch(lqmpc_handle *h, const Call &c, lqmpc::GradParams &g)
{
    int rc = grad_check(h, &c, g.Uplan, g.Xplan, g.gu0, g.gVN, g.gA, g.gB);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    rc = upload_shared(h, c, nullptr, g.so);
    if (rc) return rc;
    g.sh = (const double *)h->shared.p;
    if (!lqmpc::launch_grad(g, h->stream)) return fail(LQMPC_ERR_HIP, "lqmpc_grad_kernel launch failed");
    HIP_TRY(hipGetLastError());
    return 0;
}

// The cost-gradient calls (lqmpc_cost_grad_batch_dev, lqmpc_controller_cost_grad_dev): the checks, the shared block of `c` (the one the
// plan call before it uploaded, so nothing is copied again) and one launch of lqmpc_cost_grad_kernel -- with `reduce` on a bounded grid
// that leaves its partial sums in the handle's own block, followed by the kernel that adds them.  No solve, no plan: nothing is routed
// or compiled, and lqmpc_last_kernel is left naming the solve kernel.
static int cgrad_nulls(const void *owner, const double *Uplan, const double *Xplan, const double *gu0, const double *gVN, double *const out[7])
{
    if (!owner || !Uplan || !Xplan) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    bool any = false;
    for (int k = 0; k < 7; ++k) any = any || out[k];
    if (!any) return fail(LQMPC_ERR_BAD_ARG, "every output is NULL");
    if (!gu0 && !gVN) return fail(LQMPC_ERR_BAD_ARG, "gu0 and gVN are both NULL: there is no cotangent");
    return 0;
}

static int cgrad_check(const void *owner, const Call *c, int nx, int nu, int N, const double *Uplan, const double *Xplan, const double *gu0,
                       const double *gVN, int reduce, double *const out[7])
{
    int rc0 = cgrad_nulls(owner, Uplan, Xplan, gu0, gVN, out);
    if (rc0) return rc0;
    if (c) {                                                    // (a controller's own data passed these checks when it was made)
        const int rc = check_call(*c);
        if (rc) return rc;
    }
    if (!lqmpc::cgrad_fits(nx, nu, N, reduce ? 1 : 0)) {
        char buf[200];
        snprintf(buf, sizeof buf, "lqmpc_cost_grad_kernel needs %zu bytes of LDS at (%d,%d,%d)%s: over 160 KiB",
                 lqmpc::cgrad_lds_bytes(nx, nu, N, reduce ? 1 : 0), nx, nu, N, reduce ? " with reduce" : "");
        return fail(LQMPC_ERR_UNSUPPORTED, buf);
    }
    return 0;
}

static int cgrad_launch(lqmpc_handle *h, const Call &c, lqmpc::CGradParams &g)
{
    int rc = cgrad_check(h, &c, c.nx, c.nu, c.N, g.Uplan, g.Xplan, g.gu0, g.gVN, g.reduce, g.out);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    rc = upload_shared(h, c, nullptr, g.so);
    if (rc) return rc;
    g.sh = (const double *)h->shared.p;
    if (g.reduce) {
        rc = ensure(h, h->cgrad_part, lqmpc::cgrad_part_bytes(c.nx, c.nu, c.N, c.Bsz));
        if (rc) return rc;
        g.part = (double *)h->cgrad_part.p;
    }
    if (!lqmpc::launch_cgrad(g, h->stream)) return fail(LQMPC_ERR_HIP, "lqmpc_cost_grad_kernel launch failed");
    HIP_TRY(hipGetLastError());
    return 0;
}

// The plan-gradient calls (lqmpc_plan_grad_batch_dev, lqmpc_controller_plan_grad_dev): the checks, the shared block of `c` (the one the
// plan call before it uploaded, so nothing is copied again) and one launch of lqmpc_plan_grad_kernel.  No solve, no plan: nothing is
// routed or compiled, and lqmpc_last_kernel is left naming the solve kernel.
static int pgrad_check(const void *owner, const Call *c, int nx, int nu, int N, const double *Uplan, const double *Xplan, const double *gU,
                       const double *gX, const double *gVN, const double *gA, const double *gB, const double *gx0)
{
    if (!owner || !Uplan || !Xplan) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (!gU && !gX && !gVN) return fail(LQMPC_ERR_BAD_ARG, "gUplan, gXplan and gVN are all NULL: there is no cotangent");
    if (!gA && !gB && !gx0) return fail(LQMPC_ERR_BAD_ARG, "every output is NULL");
    if (c) {                                                    // (a controller's own data passed these checks when it was made)
        const int rc = check_call(*c);
        if (rc) return rc;
    }
    if (!lqmpc::pgrad_fits(nx, nu, N)) {
        char buf[160];
        snprintf(buf, sizeof buf, "lqmpc_plan_grad_kernel needs %zu bytes of LDS at (%d,%d,%d): over 160 KiB", lqmpc::pgrad_lds_bytes(nx, nu, N),
                 nx, nu, N);
        return fail(LQMPC_ERR_UNSUPPORTED, buf);
    }
    return 0;
}

static int pgrad_launch(lqmpc_handle *h, const Call *check, const Call &c, lqmpc::PGradParams &g)
{
    int rc = pgrad_check(h, check, c.nx, c.nu, c.N, g.Uplan, g.Xplan, g.gU, g.gX, g.gVN, g.gA, g.gB, g.gx0);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    rc = upload_shared(h, c, nullptr, g.so);
    if (rc) return rc;
    g.sh = (const double *)h->shared.p;
    if (!lqmpc::launch_pgrad(g, h->stream)) return fail(LQMPC_ERR_HIP, "lqmpc_plan_grad_kernel launch failed");
    HIP_TRY(hipGetLastError());
    return 0;
}

// the element counts of the seven outputs: per instance times Bsz, with reduce as they are
static void cgrad_counts(int nx, int nu, int N, size_t n[7])
{
    n[0] = (size_t)nx * nx; n[1] = (size_t)nu * nu; n[2] = (size_t)nx * nx; n[3] = n[4] = (size_t)nu;
    n[5] = (size_t)nx * N; n[6] = (size_t)nu * N;
}

extern "C" {

int lqmpc_reserve(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T)
{
    if (!h) return fail(LQMPC_ERR_BAD_ARG, "handle is NULL");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    if (T < 0) return fail(LQMPC_ERR_BAD_ARG, "T must be >= 0");
    HIP_TRY(hipSetDevice(h->device));
    rc = ensure(h, h->shared, 8192 * sizeof(double));
    if (rc) return rc;
    // no box, references or mode here: the plan of the widest call of this shape under the handle's options -- a rollout of T steps
    // on a per-instance plant, a one-shot solve without T -- and the buffers that call sizes
    const Call c{nx, nu, N, T, 0, T > 0 ? lqmpc::MODE_ROLLOUT : lqmpc::MODE_SOLVE, 1, Bsz};
    Plan pl;
    rc = make_plan(h->opt, c, h->device, pl);
    if (!rc && (pl.rows() || pl.family == FAM_SPEC_TIERED)) rc = ensure_fail(h, ((size_t)Bsz + FAIL_HDR) * sizeof(int));
    if (!rc && pl.order) rc = ensure_order(h, nx, nu, (size_t)Bsz, true);
    if (!rc && pl.ws_cols) rc = ensure_ws(h, c, pl);
    return rc;
}

int lqmpc_solve_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB,
                          const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                          const double *dx0, const double *x_ref, const double *u_ref, double *du0, double *dVN,
                          int32_t *dstatus, int32_t *diters)
{
    if (!h || !dA || !dB || !dx0 || !du0 || !dVN) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    return solve_dev(h, h->opt, c, dA, dB, dx0, du0, dVN, dstatus, diters);
}

int lqmpc_solve_plan_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB,
                               const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                               const double *dx0, const double *x_ref, const double *u_ref, double *du0, double *dVN,
                               double *dUplan, double *dXplan, int32_t *dstatus, int32_t *diters)
{
    if (!h || !dA || !dB || !dx0 || !du0 || !dVN || !dUplan) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    return solve_dev(h, h->opt, c, dA, dB, dx0, du0, dVN, dstatus, diters, dUplan, dXplan);
}

int lqmpc_solve_sens_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB,
                               const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                               const double *dx0, const double *x_ref, const double *u_ref, double *du0, double *dVN,
                               double *dK0, double *ddVdx, double *dKplan, double *dUplan, double *dXplan, int32_t *dstatus,
                               int32_t *diters)
{
    if (!h || !dA || !dB || !dx0 || !du0 || !dVN || !dK0 || !ddVdx) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    rc = sens_buffers(h, nx, nu, N, Bsz, dUplan, dXplan, dstatus);
    if (rc) return rc;
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    lqmpc::SensParams s{nx, nu, N, Bsz, dA, dB, Bsz, 1, dUplan, dXplan, dstatus, nullptr, {}, dK0, ddVdx, dKplan};
    rc = solve_dev(h, h->opt, c, dA, dB, dx0, du0, dVN, dstatus, diters, dUplan, dXplan, &s.so);
    return rc ? rc : sens_launch(h, s);
}

int lqmpc_model_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB,
                               const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                               const double *x_ref, const double *u_ref, const double *dUplan, const double *dXplan,
                               const int32_t *dstatus, const double *dgu0, const double *dgVN, double *dgA, double *dgB, double *dgx0)
{
    if (!h || !dA || !dB) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    lqmpc::GradParams g{nx, nu, N, Bsz, dA, dB, Bsz, 1, dUplan, dXplan, dstatus, nullptr, {}, dgu0, dgVN, dgA, dgB, dgx0};
    return grad_launch(h, c, g);
}

int lqmpc_cost_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB,
                              const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                              const double *x_ref, const double *u_ref, const double *dUplan, const double *dXplan,
                              const int32_t *dstatus, const double *dgu0, const double *dgVN, int reduce, double *dgQ, double *dgR,
                              double *dgP, double *dglb, double *dgub, double *dgxref, double *dguref, int64_t *dnskipped)
{
    if (!h || !dA || !dB) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    lqmpc::CGradParams g{nx, nu, N, Bsz, dA, dB, Bsz, 1, dUplan, dXplan, dstatus, nullptr, {}, dgu0, dgVN, reduce ? 1 : 0,
                         {dgQ, dgR, dgP, dglb, dgub, dgxref, dguref}, (long long *)dnskipped, nullptr};
    return cgrad_launch(h, c, g);
}

int lqmpc_plan_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB,
                              const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                              const double *x_ref, const double *u_ref, const double *dUplan, const double *dXplan,
                              const int32_t *dstatus, const double *dgUplan, const double *dgXplan, const double *dgVN,
                              double *dgA, double *dgB, double *dgx0)
{
    if (!h || !dA || !dB) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    lqmpc::PGradParams g{nx, nu, N, Bsz, dA, dB, Bsz, 1, dUplan, dXplan, dstatus, nullptr, {}, dgUplan, dgXplan, dgVN, dgA, dgB, dgx0};
    return pgrad_launch(h, &c, c, g);
}

int64_t lqmpc_cost_grad_blocks(int nx, int nu, int N, int64_t Bsz, int reduce)
{
    if (check_dims(nx, nu, N, Bsz)) return 0;
    return lqmpc::cgrad_blocks(nx, nu, N, Bsz, reduce ? 1 : 0);
}

int lqmpc_rollout_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *dA, const double *dB,
                            const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                            const double *dx0, const double *A_true, const double *B_true, int true_per_instance,
                            const double *x_ref, const double *u_ref, double *dJT, double *dX, double *dU,
                            int32_t *dstatus, int32_t *diters)
{
    if (!h || !dA || !dB || !dx0 || !dJT || !A_true || !B_true) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    const Call c{nx, nu, N, T, 0, lqmpc::MODE_ROLLOUT, true_per_instance ? 1 : 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref,
                 A_true, B_true, nullptr};
    return rollout_dev(h, h->opt, c, dA, dB, dx0, A_true, B_true, dJT, dX, dU, dstatus, diters);
}

// The closed loop with a tape: per step the path of lqmpc_solve_plan_batch_dev on x_t, its plan written into slice t of the tape, and
// one launch of lqmpc_plant_step_kernel behind it.  The shared block is that of a solve with the shared plant in its At, Bt slots
// (a solve kernel never reads them), so it is packed T times, compared T times and uploaded once.
int lqmpc_rollout_tape_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *dA, const double *dB,
                                 const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                                 const double *dx0, const double *A_true, const double *B_true, int true_per_instance,
                                 const double *x_ref, const double *u_ref, double *dJT, double *dX, double *dU,
                                 int32_t *dstatus, int32_t *diters, double *dUtape, int32_t *dstatus_tape)
{
    if (!h || !dA || !dB || !dx0 || !dJT || !A_true || !B_true || !dUtape) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    const bool per = true_per_instance != 0;
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, per ? nullptr : A_true, per ? nullptr : B_true,
                 nullptr};
    int rc = check_call(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    // the handle's block: [x of two steps | u_0 | V_N] in doubles, then [status | iters] of one solve
    const size_t b = (size_t)Bsz, dbl = b * (2 * (size_t)nx + nu + 1);
    rc = ensure(h, h->tape, dbl * sizeof(double) + 2 * b * sizeof(int32_t));
    if (rc) return rc;
    double *xb[2] = {(double *)h->tape.p, (double *)h->tape.p + b * nx};
    double *u0 = xb[1] + b * nx, *vn = u0 + b * nu;
    int32_t *st = (int32_t *)(vn + b), *it = st + b;
    const size_t slice = b * nu * N;
    for (int t = 0; t < T; ++t) {
        const double *x = t == 0 ? dx0 : xb[t & 1];
        int32_t *st_t = dstatus_tape ? dstatus_tape + (size_t)t * b : st;
        lqmpc::SharedOff so;
        rc = solve_dev(h, h->opt, c, dA, dB, x, u0, vn, st_t, it, dUtape + (size_t)t * slice, nullptr, &so);
        if (rc) return rc;
        const double *sh = (const double *)h->shared.p;
        lqmpc::PlantStepParams s{nx, nu, N, T, t, Bsz, per ? A_true : sh + so.At, per ? B_true : sh + so.Bt, per ? Bsz : 1, per ? 1 : 0,
                                 sh, so, x, dUtape + (size_t)t * slice, st_t, it, xb[(t + 1) & 1], dJT, dX, dU, dstatus, diters};
        lqmpc::launch_plant_step(s, h->stream);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// The gradient of that loop: the checks, the shared block of the tape call (so nothing is copied again) and one launch of
// lqmpc_rollout_grad_kernel.  No solve: nothing is routed or compiled, and lqmpc_last_kernel is left naming the solve kernel.
static int rgrad_check(const void *h, const Call &c, int T, const double *A, const double *B, const double *At, const double *Bt,
                       const double *X, const double *Utape, const double *gJT, const double *gX, const double *gU, const double *gA,
                       const double *gB, const double *gx0, const double *gAt, const double *gBt)
{
    if (!h || !A || !B || !At || !Bt || !X || !Utape) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (!gJT && !gX && !gU) return fail(LQMPC_ERR_BAD_ARG, "gJT, gX and gU are all NULL: there is no cotangent");
    if (!gA && !gB && !gx0 && !gAt && !gBt) return fail(LQMPC_ERR_BAD_ARG, "every output is NULL");
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    const int rc = check_call(c);
    if (rc) return rc;
    if (!lqmpc::rgrad_fits(c.nx, c.nu, c.N)) {
        char buf[160];
        snprintf(buf, sizeof buf, "lqmpc_rollout_grad_kernel needs %zu bytes of LDS at (%d,%d,%d): over 160 KiB",
                 lqmpc::rgrad_lds_bytes(c.nx, c.nu, c.N), c.nx, c.nu, c.N);
        return fail(LQMPC_ERR_UNSUPPORTED, buf);
    }
    return 0;
}

int lqmpc_rollout_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *dA, const double *dB,
                                 const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                                 const double *A_true, const double *B_true, int true_per_instance, const double *x_ref,
                                 const double *u_ref, const double *dX, const double *dUtape, const int32_t *dstatus_tape,
                                 const double *dgJT, const double *dgX, const double *dgU, double *dgA, double *dgB, double *dgx0,
                                 double *dgA_true, double *dgB_true)
{
    const bool per = true_per_instance != 0;
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, per ? nullptr : A_true, per ? nullptr : B_true,
                 nullptr};
    int rc = rgrad_check(h, c, T, dA, dB, A_true, B_true, dX, dUtape, dgJT, dgX, dgU, dgA, dgB, dgx0, dgA_true, dgB_true);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    lqmpc::RGradParams g{};
    rc = upload_shared(h, c, nullptr, g.so);
    if (rc) return rc;
    const double *sh = (const double *)h->shared.p;
    g.nx = nx; g.nu = nu; g.N = N; g.T = T; g.Bsz = Bsz;
    g.A = dA; g.B = dB;
    g.At = per ? A_true : sh + g.so.At; g.Bt = per ? B_true : sh + g.so.Bt;
    g.sE = per ? Bsz : 1; g.sI = per ? 1 : 0;
    g.X = dX; g.Utape = dUtape; g.status_tape = dstatus_tape; g.sh = sh;
    g.gJT = dgJT; g.gX = dgX; g.gU = dgU;
    g.gA = dgA; g.gB = dgB; g.gx0 = dgx0; g.gAt = dgA_true; g.gBt = dgB_true;
    if (!lqmpc::launch_rgrad(g, h->stream)) return fail(LQMPC_ERR_HIP, "lqmpc_rollout_grad_kernel launch failed");
    HIP_TRY(hipGetLastError());
    return 0;
}

// The gradient of that loop in the data the batch shares: the checks, the shared block of the tape call and one launch of
// lqmpc_rollout_cost_grad_kernel -- with `reduce` followed by the kernel that adds the wavefronts' partial sums, which lie in a block
// of the handle's own.  No solve: nothing is routed or compiled, and lqmpc_last_kernel is left naming the solve kernel.
static int rcgrad_check(const void *h, const Call &c, int T, const double *A, const double *B, const double *At, const double *Bt,
                        const double *X, const double *Utape, const double *gJT, const double *gX, const double *gU, double *const out[7])
{
    if (!h || !A || !B || !At || !Bt || !X || !Utape) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (!gJT && !gX && !gU) return fail(LQMPC_ERR_BAD_ARG, "gJT, gX and gU are all NULL: there is no cotangent");
    bool any = false;
    for (int k = 0; k < 7; ++k) any = any || out[k];
    if (!any) return fail(LQMPC_ERR_BAD_ARG, "every output is NULL");
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    const int rc = check_call(c);
    if (rc) return rc;
    if (!lqmpc::rcgrad_fits(c.nx, c.nu, c.N)) {
        char buf[160];
        snprintf(buf, sizeof buf, "lqmpc_rollout_cost_grad_kernel needs %zu bytes of LDS at (%d,%d,%d): over 160 KiB",
                 lqmpc::rcgrad_lds_bytes(c.nx, c.nu, c.N), c.nx, c.nu, c.N);
        return fail(LQMPC_ERR_UNSUPPORTED, buf);
    }
    return 0;
}

int lqmpc_rollout_cost_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *dA, const double *dB,
                                      const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                                      const double *A_true, const double *B_true, int true_per_instance, const double *x_ref,
                                      const double *u_ref, const double *dX, const double *dUtape, const int32_t *dstatus_tape,
                                      const double *dgJT, const double *dgX, const double *dgU, int reduce, double *dgQ, double *dgR,
                                      double *dgP, double *dglb, double *dgub, double *dgxref, double *dguref, int64_t *dnskipped)
{
    const bool per = true_per_instance != 0;
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, per ? nullptr : A_true, per ? nullptr : B_true,
                 nullptr};
    lqmpc::RCGradParams g{};
    double *const outs[7] = {dgQ, dgR, dgP, dglb, dgub, dgxref, dguref};
    int rc = rcgrad_check(h, c, T, dA, dB, A_true, B_true, dX, dUtape, dgJT, dgX, dgU, outs);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    rc = upload_shared(h, c, nullptr, g.so);
    if (rc) return rc;
    const double *sh = (const double *)h->shared.p;
    g.nx = nx; g.nu = nu; g.N = N; g.T = T; g.Bsz = Bsz;
    g.A = dA; g.B = dB;
    g.At = per ? A_true : sh + g.so.At; g.Bt = per ? B_true : sh + g.so.Bt;
    g.sE = per ? Bsz : 1; g.sI = per ? 1 : 0;
    g.X = dX; g.Utape = dUtape; g.status_tape = dstatus_tape; g.sh = sh;
    g.gJT = dgJT; g.gX = dgX; g.gU = dgU;
    g.reduce = reduce ? 1 : 0;
    for (int k = 0; k < 7; ++k) g.out[k] = outs[k];
    g.nskipped = (long long *)dnskipped;
    if (g.reduce) {
        rc = ensure(h, h->rcgrad_part, lqmpc::rcgrad_part_bytes(nx, nu, N, Bsz));
        if (rc) return rc;
        g.part = (double *)h->rcgrad_part.p;
    }
    if (!lqmpc::launch_rcgrad(g, h->stream)) return fail(LQMPC_ERR_HIP, "lqmpc_rollout_cost_grad_kernel launch failed");
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---- polytopic input constraints Fu u <= 1 (lqmpc_poly.hip) ----
constexpr int POLY_MAX_NVAR = 64, POLY_MAX_ROWS = 16;

// Every refusal of a polytope call, from the arguments alone: the handle is not dereferenced, nothing is enqueued.
static int poly_check(const void *h, int nx, int nu, int N, int64_t Bsz, int T, bool roll, const double *A, const double *B, const double *Q,
                      const double *R, const double *P, const double *Fu, int m, const double *x0, const double *At, const double *Bt,
                      int max_iter, const void *out0, const void *out1)
{
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    if (m < 1) return fail(LQMPC_ERR_BAD_ARG, "m must be positive: Fu needs at least one row");
    if (N * nu > POLY_MAX_NVAR || m > POLY_MAX_ROWS || !lqmpc::poly_fits(nx, nu, N, m)) {
        char buf[256];
        snprintf(buf, sizeof buf, "the polytope kernels serve nx<=%d, nu<=%d, N<=%d, N*nu<=%d, 1<=m<=%d and an LDS image within 160 KiB; "
                 "(%d,%d,%d) with m=%d (LDS %zu bytes) is outside", LQMPC_MAX_NX, LQMPC_MAX_NU, LQMPC_MAX_N, POLY_MAX_NVAR, POLY_MAX_ROWS,
                 nx, nu, N, m, m <= POLY_MAX_ROWS ? lqmpc::poly_lds_bytes(nx, nu, N, m) : (size_t)0);
        return fail(LQMPC_ERR_UNSUPPORTED, buf);
    }
    if (!h || !A || !B || !x0 || !out0 || !out1 || (roll && (!At || !Bt))) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (!Q || !R || !P || !Fu) return fail(LQMPC_ERR_BAD_ARG, "Q, R, P, Fu must not be NULL");
    if (roll && (T < 1 || T > 100000)) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    if (max_iter < 0) return fail(LQMPC_ERR_BAD_ARG, "max_iter must be >= 0 (0: 10 N nu + 20)");
    for (int j = 0; j < m; ++j) {
        bool zero = true;
        for (int k = 0; k < nu; ++k) {
            if (!std::isfinite(Fu[j * nu + k])) {
                char buf[96];
                snprintf(buf, sizeof buf, "row %d of Fu holds a non-finite entry", j);
                return fail(LQMPC_ERR_BAD_ARG, buf);
            }
            zero = zero && Fu[j * nu + k] == 0.0;
        }
        if (zero) {
            char buf[96];
            snprintf(buf, sizeof buf, "row %d of Fu is all zero", j);
            return fail(LQMPC_ERR_BAD_ARG, buf);
        }
    }
    return 0;
}

// The shared block of a polytope call, the parameter block and the one launch.
static int poly_run(lqmpc_handle *h, lqmpc::PolyParams &p, const double *Q, const double *R, const double *P, const double *Fu,
                    const double *x_ref, const double *u_ref, const double *At_sh, const double *Bt_sh)
{
    HIP_TRY(hipSetDevice(h->device));
    const int nx = p.nx, nu = p.nu, N = p.N;
    std::vector<double> sh;
    auto put = [&](const double *src, int count) {
        int off = (int)sh.size();
        sh.resize(sh.size() + count, 0.0);
        if (src) memcpy(sh.data() + off, src, sizeof(double) * count);
        return off;
    };
    p.so.Q = put(Q, nx * nx);
    p.so.R = put(R, nu * nu);
    p.so.P = put(P, nx * nx);
    p.so.Fu = put(Fu, p.m * nu);
    p.so.xref = put(x_ref, nx * N);
    p.so.uref = put(u_ref, nu * N);
    p.so.At = put(At_sh, nx * nx);
    p.so.Bt = put(Bt_sh, nx * nu);
    const int rc = upload_block(h, sh);
    if (rc) return rc;
    p.sh = (const double *)h->shared.p;
    if (At_sh) { p.At = p.sh + p.so.At; p.Bt = p.sh + p.so.Bt; p.sE = 1; p.sI = 0; }
    p.eps = h->opt.eps;
    const char *name = nullptr;
    if (!lqmpc::launch_poly(p, h->stream, &name)) return fail(LQMPC_ERR_HIP, "the polytope kernel's launch failed");
    HIP_TRY(hipGetLastError());
    set_last_kernel(h, name);
    return 0;
}

extern "C" {

int lqmpc_solve_poly_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB, const double *Q,
                               const double *R, const double *P, const double *Fu, int m, const double *dx0, const double *x_ref,
                               const double *u_ref, int max_iter, double *du0, double *dVN, double *dUplan, double *dXplan, double *dlam,
                               int32_t *dstatus, int32_t *diters)
{
    const int rc = poly_check(h, nx, nu, N, Bsz, 0, false, dA, dB, Q, R, P, Fu, m, dx0, nullptr, nullptr, max_iter, du0, dVN);
    if (rc) return rc;
    lqmpc::PolyParams p{};
    p.nx = nx; p.nu = nu; p.N = N; p.m = m; p.T = 0; p.max_iter = max_iter; p.Bsz = Bsz;
    p.A = dA; p.B = dB; p.x0 = dx0;
    p.u0 = du0; p.VN = dVN; p.Uplan = dUplan; p.Xplan = dXplan; p.lam = dlam; p.status = dstatus; p.iters = diters;
    return poly_run(h, p, Q, R, P, Fu, x_ref, u_ref, nullptr, nullptr);
}

int lqmpc_rollout_poly_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *dA, const double *dB,
                                 const double *Q, const double *R, const double *P, const double *Fu, int m, const double *dx0,
                                 const double *A_true, const double *B_true, int true_per_instance, const double *x_ref,
                                 const double *u_ref, int max_iter, double *dJT, double *dX, double *dU, int32_t *dstatus, int32_t *diters)
{
    const int rc = poly_check(h, nx, nu, N, Bsz, T, true, dA, dB, Q, R, P, Fu, m, dx0, A_true, B_true, max_iter, dJT, dJT);
    if (rc) return rc;
    const bool per = true_per_instance != 0;
    lqmpc::PolyParams p{};
    p.nx = nx; p.nu = nu; p.N = N; p.m = m; p.T = T; p.max_iter = max_iter; p.Bsz = Bsz;
    p.A = dA; p.B = dB; p.x0 = dx0;
    p.At = A_true; p.Bt = B_true; p.sE = Bsz; p.sI = 1;       // per instance; poly_run points a shared plant into the shared block
    p.JT = dJT; p.X = dX; p.U = dU; p.status = dstatus; p.iters = diters;
    return poly_run(h, p, Q, R, P, Fu, x_ref, u_ref, per ? nullptr : A_true, per ? nullptr : B_true);
}

int lqmpc_max_vn_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int K, const double *dA, const double *dB,
                           const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                           const double *x0s, const double *x_ref, const double *u_ref, double *dMV, int32_t *dstatus,
                           int32_t *diters)
{
    if (!h || !dA || !dB || !x0s || !dMV) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (K < 1 || K > 1024) return fail(LQMPC_ERR_BAD_ARG, "K must be in [1,1024]");
    Call c{nx, nu, N, 0, K, lqmpc::MODE_MAXVN, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, x0s};
    KParams p;
    Plan pl;
    int rc = prepare(h, h->opt, c, p, pl);
    if (rc) return rc;
    p.A = dA; p.B = dB; p.MV = dMV; p.status = dstatus; p.iters = diters;
    return run(h, pl, p);
}

int lqmpc_sweep_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, int K, const double *dA, const double *dB,
                          const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                          const double *dx0, const double *x0s, const double *A_true, const double *B_true,
                          int true_per_instance, const double *x_ref, const double *u_ref, double *dJT, double *dMV,
                          int32_t *dstatus, int32_t *diters)
{
    if (!h || !dA || !dB || !dx0 || !x0s || !dJT || !dMV || !A_true || !B_true) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    if (K < 1 || K > 1024) return fail(LQMPC_ERR_BAD_ARG, "K must be in [1,1024]");
    Call c{nx, nu, N, T, K, lqmpc::MODE_SWEEP, true_per_instance ? 1 : 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, A_true, B_true, x0s};
    KParams p;
    Plan pl;
    int rc = prepare(h, h->opt, c, p, pl);
    if (rc) return rc;
    if (pl.rows()) {
        // one launch: condensing and W once per instance, K open-loop QPs, then the closed loop
        p.A = dA; p.B = dB; p.x0 = dx0; p.JT = dJT; p.MV = dMV; p.status = dstatus; p.iters = diters;
        if (true_per_instance) { p.At = A_true; p.Bt = B_true; }
        return run(h, pl, p);
    }
    // no fused kernel for this shape / size: the two launches (each plans for itself), status = worse of the two, iters = their sum
    int32_t *st2 = nullptr, *it2 = nullptr;
    if (dstatus) { rc = ensure(h, h->st2, (size_t)Bsz * sizeof(int32_t)); if (rc) return rc; st2 = (int32_t *)h->st2.p; }
    if (diters) { rc = ensure(h, h->it2, (size_t)Bsz * sizeof(int32_t)); if (rc) return rc; it2 = (int32_t *)h->it2.p; }
    rc = lqmpc_max_vn_batch_dev(h, nx, nu, N, Bsz, K, dA, dB, Q, R, P, lb, ub, x0s, x_ref, u_ref, dMV, st2, it2);
    if (rc) return rc;
    rc = lqmpc_rollout_batch_dev(h, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, dx0, A_true, B_true, true_per_instance, x_ref, u_ref,
                                 dJT, nullptr, nullptr, dstatus, diters);
    if (rc) return rc;
    if (dstatus || diters) {
        hipLaunchKernelGGL(lqmpc_merge_status_kernel, dim3((unsigned)((Bsz + 255) / 256)), dim3(256), 0, h->stream, dstatus, diters,
                           st2, it2, (long long)Bsz);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // extern "C"

// ---- host-buffer flavours: stage in, run, stage out ----
namespace {
// An entry point names each of its arrays once -- in() / out() with the host pointer, the element count and the variable that takes
// the device pointer -- then upload(), the launches, finish().  From upload() on the variables hold the device addresses (NULL for a
// NULL host pointer, which is not copied either); finish() brings the outputs back and waits for the stream.  All arrays of a call
// share one device block laid out by lqmpc::ArenaLayout, which grows as needed.
// Small calls (the reference's own call shape is ONE instance per solve(), utils_class.py:269) are dominated by the number of
// copies, not their size: up to PACK_LIMIT bytes in total the block has a pinned host image -- one copy in, one copy out.  Larger
// calls copy array by array straight from / to the caller's buffers.
constexpr size_t PACK_LIMIT = 256 * 1024;
struct Stager {
    lqmpc_handle *h;
    lqmpc::ArenaLayout lay;
    struct Arr { void *host; void *var; void (*set)(void *var, char *dev); };
    std::vector<Arr> arrs;                                        // one per slot of lay
    bool may_pack = true;                                         // false: array by array whatever the size
    bool packed = false;

    template <typename T>
    void add(T *host, size_t count, T *&dev, bool out)
    {
        dev = nullptr;
        if (arrs.empty()) { arrs.reserve(16); lay.slots.reserve(16); }      // (one allocation each for every entry point there is)
        lay.add(count * sizeof(T), out, host != nullptr);
        arrs.push_back(Arr{(void *)host, &dev, [](void *var, char *d) { *(T **)var = (T *)d; }});
    }
    template <typename T> void in(const T *host, size_t count, const T *&dev) { add(host, count, dev, false); }
    template <typename T> void out(T *host, size_t count, T *&dev) { add(host, count, dev, true); }
    int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, const char *what)
    {
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
        return e == hipSuccess ? 0 : fail(LQMPC_ERR_HIP, std::string(what) + hipGetErrorString(e));
    }
    // after the last in() / out(): room for everything, the inputs on their way
    int upload()
    {
        lay.place();
        packed = may_pack && lay.total <= PACK_LIMIT;
        int rc = ensure(h, h->arena, lay.total);
        if (!rc && packed) rc = ensure_host(h->arena_pin, lay.total);
        char *dev = (char *)h->arena.p, *pin = (char *)h->arena_pin.p;
        for (size_t k = 0; !rc && k < arrs.size(); ++k) {
            const lqmpc::ArenaLayout::Slot &sl = lay.slots[k];
            if (!sl.present) continue;
            arrs[k].set(arrs[k].var, dev + sl.off);
            if (sl.out) continue;
            if (packed) memcpy(pin + sl.off, arrs[k].host, sl.bytes);
            else rc = copy(dev + sl.off, arrs[k].host, sl.bytes, hipMemcpyHostToDevice, "H2D: ");
        }
        if (!rc && packed && lay.in_end) rc = copy(dev, pin, lay.in_end, hipMemcpyHostToDevice, "H2D: ");
        return rc;
    }
    // after the launches: the outputs on their way back, the wait, and (packed) the hand-over to the caller's arrays
    int finish()
    {
        char *dev = (char *)h->arena.p, *pin = (char *)h->arena_pin.p;
        int rc = 0;
        if (packed && lay.total > lay.in_end) rc = copy(pin + lay.in_end, dev + lay.in_end, lay.total - lay.in_end, hipMemcpyDeviceToHost, "D2H: ");
        for (size_t k = 0; !packed && !rc && k < arrs.size(); ++k)
            if (lay.slots[k].present && lay.slots[k].out) rc = copy(arrs[k].host, dev + lay.slots[k].off, lay.slots[k].bytes, hipMemcpyDeviceToHost, "D2H: ");
        if (rc) return rc;
        const hipError_t e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(LQMPC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
        for (size_t k = 0; packed && k < arrs.size(); ++k)
            if (lay.slots[k].present && lay.slots[k].out) memcpy(arrs[k].host, pin + lay.slots[k].off, lay.slots[k].bytes);
        return 0;
    }
};
}  // namespace

extern "C" {

int lqmpc_solve_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B,
                      const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                      const double *x0, const double *x_ref, const double *u_ref, double *u0, double *VN,
                      int32_t *status, int32_t *iters)
{
    if (!h || !A || !B || !x0 || !u0 || !VN) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dx0;
    double *du0, *dVN;
    int32_t *dst, *dit;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(x0, b * nx, dx0);
    s.out(u0, b * nu, du0); s.out(VN, b, dVN); s.out(status, b, dst); s.out(iters, b, dit);
    rc = s.upload();
    if (!rc) rc = lqmpc_solve_batch_dev(h, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, dx0, x_ref, u_ref, du0, dVN, dst, dit);
    return rc ? rc : s.finish();
}

int lqmpc_solve_plan_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B,
                           const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                           const double *x0, const double *x_ref, const double *u_ref, double *u0, double *VN,
                           double *Uplan, double *Xplan, int32_t *status, int32_t *iters)
{
    if (!h || !A || !B || !x0 || !u0 || !VN || !Uplan) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dx0;
    double *du0, *dVN, *dUp, *dXp;
    int32_t *dst, *dit;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(x0, b * nx, dx0);
    s.out(u0, b * nu, du0); s.out(VN, b, dVN); s.out(Uplan, b * nu * N, dUp); s.out(Xplan, b * nx * (N + 1), dXp);
    s.out(status, b, dst); s.out(iters, b, dit);
    rc = s.upload();
    if (!rc) rc = lqmpc_solve_plan_batch_dev(h, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, dx0, x_ref, u_ref, du0, dVN, dUp, dXp, dst, dit);
    return rc ? rc : s.finish();
}

int lqmpc_solve_sens_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B,
                           const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                           const double *x0, const double *x_ref, const double *u_ref, double *u0, double *VN,
                           double *K0, double *dVdx, double *Kplan, double *Uplan, double *Xplan, int32_t *status, int32_t *iters)
{
    if (!h || !A || !B || !x0 || !u0 || !VN || !K0 || !dVdx) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dx0;
    double *du0, *dVN, *dK0, *ddV, *dKp, *dUp, *dXp;
    int32_t *dst, *dit;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(x0, b * nx, dx0);
    s.out(u0, b * nu, du0); s.out(VN, b, dVN); s.out(K0, b * nu * nx, dK0); s.out(dVdx, b * nx, ddV);
    s.out(Kplan, b * nu * N * nx, dKp); s.out(Uplan, b * nu * N, dUp); s.out(Xplan, b * nx * (N + 1), dXp);
    s.out(status, b, dst); s.out(iters, b, dit);
    rc = s.upload();
    if (!rc) rc = lqmpc_solve_sens_batch_dev(h, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, dx0, x_ref, u_ref, du0, dVN, dK0, ddV, dKp, dUp, dXp,
                                             dst, dit);
    return rc ? rc : s.finish();
}

int lqmpc_model_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B,
                           const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                           const double *x_ref, const double *u_ref, const double *Uplan, const double *Xplan, const int32_t *status,
                           const double *gu0, const double *gVN, double *gA, double *gB, double *gx0)
{
    if (!A || !B) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    int rc = grad_check(h, &c, Uplan, Xplan, gu0, gVN, gA, gB);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dUp, *dXp, *dgu, *dgV;
    const int32_t *dst;
    double *dgA, *dgB, *dgx;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(Uplan, b * nu * N, dUp); s.in(Xplan, b * nx * (N + 1), dXp);
    s.in(status, b, dst); s.in(gu0, b * nu, dgu); s.in(gVN, b, dgV);
    s.out(gA, b * nx * nx, dgA); s.out(gB, b * nx * nu, dgB); s.out(gx0, b * nx, dgx);
    rc = s.upload();
    if (!rc) rc = lqmpc_model_grad_batch_dev(h, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, x_ref, u_ref, dUp, dXp, dst, dgu, dgV, dgA, dgB, dgx);
    return rc ? rc : s.finish();
}

int lqmpc_cost_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B,
                          const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                          const double *x_ref, const double *u_ref, const double *Uplan, const double *Xplan, const int32_t *status,
                          const double *gu0, const double *gVN, int reduce, double *gQ, double *gR, double *gP, double *glb, double *gub,
                          double *gxref, double *guref, int64_t *nskipped)
{
    if (!A || !B) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    double *const outs[7] = {gQ, gR, gP, glb, gub, gxref, guref};
    int rc = cgrad_check(h, &c, nx, nu, N, Uplan, Xplan, gu0, gVN, reduce, outs);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz, per = reduce ? 1 : b;
    size_t n[7];
    cgrad_counts(nx, nu, N, n);
    const double *dA, *dB, *dUp, *dXp, *dgu, *dgV;
    const int32_t *dst;
    double *d[7];
    int64_t *dns;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(Uplan, b * nu * N, dUp); s.in(Xplan, b * nx * (N + 1), dXp);
    s.in(status, b, dst); s.in(gu0, b * nu, dgu); s.in(gVN, b, dgV);
    for (int k = 0; k < 7; ++k) s.out(outs[k], n[k] * per, d[k]);
    s.out(reduce ? nskipped : (int64_t *)nullptr, 1, dns);
    rc = s.upload();
    if (!rc) rc = lqmpc_cost_grad_batch_dev(h, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, x_ref, u_ref, dUp, dXp, dst, dgu, dgV, reduce,
                                            d[0], d[1], d[2], d[3], d[4], d[5], d[6], dns);
    return rc ? rc : s.finish();
}

int lqmpc_plan_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B,
                          const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                          const double *x_ref, const double *u_ref, const double *Uplan, const double *Xplan, const int32_t *status,
                          const double *gUplan, const double *gXplan, const double *gVN, double *gA, double *gB, double *gx0)
{
    if (!A || !B) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    int rc = pgrad_check(h, &c, nx, nu, N, Uplan, Xplan, gUplan, gXplan, gVN, gA, gB, gx0);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dUp, *dXp, *dgU, *dgX, *dgV;
    const int32_t *dst;
    double *dgA, *dgB, *dgx;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(Uplan, b * nu * N, dUp); s.in(Xplan, b * nx * (N + 1), dXp);
    s.in(status, b, dst); s.in(gUplan, b * nu * N, dgU); s.in(gXplan, b * nx * (N + 1), dgX); s.in(gVN, b, dgV);
    s.out(gA, b * nx * nx, dgA); s.out(gB, b * nx * nu, dgB); s.out(gx0, b * nx, dgx);
    rc = s.upload();
    if (!rc) rc = lqmpc_plan_grad_batch_dev(h, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, x_ref, u_ref, dUp, dXp, dst, dgU, dgX, dgV, dgA, dgB, dgx);
    return rc ? rc : s.finish();
}

int lqmpc_rollout_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *A, const double *B,
                        const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                        const double *x0, const double *A_true, const double *B_true, int true_per_instance,
                        const double *x_ref, const double *u_ref, double *JT, double *X, double *U, int32_t *status,
                        int32_t *iters)
{
    if (!h || !A || !B || !x0 || !JT || !A_true || !B_true) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dx0, *dAt = A_true, *dBt = B_true;
    double *dJT, *dX, *dU;
    int32_t *dst, *dit;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(x0, b * nx, dx0);
    if (true_per_instance) { s.in(A_true, b * nx * nx, dAt); s.in(B_true, b * nx * nu, dBt); }
    s.out(JT, b, dJT); s.out(X, b * nx * (T + 1), dX); s.out(U, b * nu * T, dU); s.out(status, b, dst); s.out(iters, b, dit);
    rc = s.upload();
    if (!rc) rc = lqmpc_rollout_batch_dev(h, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, dx0, dAt, dBt, true_per_instance, x_ref,
                                          u_ref, dJT, dX, dU, dst, dit);
    return rc ? rc : s.finish();
}

int lqmpc_rollout_tape_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *A, const double *B,
                             const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                             const double *x0, const double *A_true, const double *B_true, int true_per_instance,
                             const double *x_ref, const double *u_ref, double *JT, double *X, double *U, int32_t *status,
                             int32_t *iters, double *Utape, int32_t *status_tape)
{
    if (!h || !A || !B || !x0 || !JT || !A_true || !B_true || !Utape) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dx0, *dAt = A_true, *dBt = B_true;
    double *dJT, *dX, *dU, *dUt;
    int32_t *dst, *dit, *dstt;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(x0, b * nx, dx0);
    if (true_per_instance) { s.in(A_true, b * nx * nx, dAt); s.in(B_true, b * nx * nu, dBt); }
    s.out(JT, b, dJT); s.out(X, b * nx * (T + 1), dX); s.out(U, b * nu * T, dU); s.out(status, b, dst); s.out(iters, b, dit);
    s.out(Utape, b * nu * N * T, dUt); s.out(status_tape, b * T, dstt);
    rc = s.upload();
    if (!rc) rc = lqmpc_rollout_tape_batch_dev(h, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, dx0, dAt, dBt, true_per_instance, x_ref,
                                               u_ref, dJT, dX, dU, dst, dit, dUt, dstt);
    return rc ? rc : s.finish();
}

int lqmpc_rollout_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *A, const double *B,
                             const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                             const double *A_true, const double *B_true, int true_per_instance, const double *x_ref,
                             const double *u_ref, const double *X, const double *Utape, const int32_t *status_tape, const double *gJT,
                             const double *gX, const double *gU, double *gA, double *gB, double *gx0, double *gA_true, double *gB_true)
{
    const bool per = true_per_instance != 0;
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, per ? nullptr : A_true, per ? nullptr : B_true,
                 nullptr};
    int rc = rgrad_check(h, c, T, A, B, A_true, B_true, X, Utape, gJT, gX, gU, gA, gB, gx0, gA_true, gB_true);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dAt = A_true, *dBt = B_true, *dX, *dUt, *dgJ, *dgX, *dgU;
    const int32_t *dstt;
    double *dgA, *dgB, *dgx, *dgAt, *dgBt;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB);
    if (per) { s.in(A_true, b * nx * nx, dAt); s.in(B_true, b * nx * nu, dBt); }
    s.in(X, b * nx * (T + 1), dX); s.in(Utape, b * nu * N * T, dUt); s.in(status_tape, b * T, dstt);
    s.in(gJT, b, dgJ); s.in(gX, b * nx * (T + 1), dgX); s.in(gU, b * nu * T, dgU);
    s.out(gA, b * nx * nx, dgA); s.out(gB, b * nx * nu, dgB); s.out(gx0, b * nx, dgx);
    s.out(gA_true, b * nx * nx, dgAt); s.out(gB_true, b * nx * nu, dgBt);
    rc = s.upload();
    if (!rc) rc = lqmpc_rollout_grad_batch_dev(h, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, dAt, dBt, true_per_instance, x_ref, u_ref, dX,
                                               dUt, dstt, dgJ, dgX, dgU, dgA, dgB, dgx, dgAt, dgBt);
    return rc ? rc : s.finish();
}

int lqmpc_rollout_cost_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *A, const double *B,
                                  const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                                  const double *A_true, const double *B_true, int true_per_instance, const double *x_ref,
                                  const double *u_ref, const double *X, const double *Utape, const int32_t *status_tape,
                                  const double *gJT, const double *gX, const double *gU, int reduce, double *gQ, double *gR, double *gP,
                                  double *glb, double *gub, double *gxref, double *guref, int64_t *nskipped)
{
    const bool per = true_per_instance != 0;
    const Call c{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, per ? nullptr : A_true, per ? nullptr : B_true,
                 nullptr};
    double *const outs[7] = {gQ, gR, gP, glb, gub, gxref, guref};
    int rc = rcgrad_check(h, c, T, A, B, A_true, B_true, X, Utape, gJT, gX, gU, outs);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz, cnt = reduce ? 1 : b;
    size_t n[7];
    cgrad_counts(nx, nu, N, n);
    const double *dA, *dB, *dAt = A_true, *dBt = B_true, *dX, *dUt, *dgJ, *dgX, *dgU;
    const int32_t *dstt;
    double *d[7];
    int64_t *dns;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB);
    if (per) { s.in(A_true, b * nx * nx, dAt); s.in(B_true, b * nx * nu, dBt); }
    s.in(X, b * nx * (T + 1), dX); s.in(Utape, b * nu * N * T, dUt); s.in(status_tape, b * T, dstt);
    s.in(gJT, b, dgJ); s.in(gX, b * nx * (T + 1), dgX); s.in(gU, b * nu * T, dgU);
    for (int k = 0; k < 7; ++k) s.out(outs[k], n[k] * cnt, d[k]);
    s.out(reduce ? nskipped : (int64_t *)nullptr, 1, dns);
    rc = s.upload();
    if (!rc) rc = lqmpc_rollout_cost_grad_batch_dev(h, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, dAt, dBt, true_per_instance, x_ref, u_ref,
                                                    dX, dUt, dstt, dgJ, dgX, dgU, reduce, d[0], d[1], d[2], d[3], d[4], d[5], d[6], dns);
    return rc ? rc : s.finish();
}

int lqmpc_solve_poly_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B, const double *Q,
                           const double *R, const double *P, const double *Fu, int m, const double *x0, const double *x_ref,
                           const double *u_ref, int max_iter, double *u0, double *VN, double *Uplan, double *Xplan, double *lam,
                           int32_t *status, int32_t *iters)
{
    int rc = poly_check(h, nx, nu, N, Bsz, 0, false, A, B, Q, R, P, Fu, m, x0, nullptr, nullptr, max_iter, u0, VN);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dx0;
    double *du0, *dVN, *dUp, *dXp, *dlam;
    int32_t *dst, *dit;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(x0, b * nx, dx0);
    s.out(u0, b * nu, du0); s.out(VN, b, dVN); s.out(Uplan, b * nu * N, dUp); s.out(Xplan, b * nx * (N + 1), dXp);
    s.out(lam, b * m * N, dlam); s.out(status, b, dst); s.out(iters, b, dit);
    rc = s.upload();
    if (!rc) rc = lqmpc_solve_poly_batch_dev(h, nx, nu, N, Bsz, dA, dB, Q, R, P, Fu, m, dx0, x_ref, u_ref, max_iter, du0, dVN, dUp, dXp, dlam,
                                             dst, dit);
    return rc ? rc : s.finish();
}

int lqmpc_rollout_poly_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, const double *A, const double *B,
                             const double *Q, const double *R, const double *P, const double *Fu, int m, const double *x0,
                             const double *A_true, const double *B_true, int true_per_instance, const double *x_ref,
                             const double *u_ref, int max_iter, double *JT, double *X, double *U, int32_t *status, int32_t *iters)
{
    int rc = poly_check(h, nx, nu, N, Bsz, T, true, A, B, Q, R, P, Fu, m, x0, A_true, B_true, max_iter, JT, JT);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dx0, *dAt = A_true, *dBt = B_true;
    double *dJT, *dX, *dU;
    int32_t *dst, *dit;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(x0, b * nx, dx0);
    if (true_per_instance) { s.in(A_true, b * nx * nx, dAt); s.in(B_true, b * nx * nu, dBt); }
    s.out(JT, b, dJT); s.out(X, b * nx * (T + 1), dX); s.out(U, b * nu * T, dU); s.out(status, b, dst); s.out(iters, b, dit);
    rc = s.upload();
    if (!rc) rc = lqmpc_rollout_poly_batch_dev(h, nx, nu, N, Bsz, T, dA, dB, Q, R, P, Fu, m, dx0, dAt, dBt, true_per_instance, x_ref,
                                               u_ref, max_iter, dJT, dX, dU, dst, dit);
    return rc ? rc : s.finish();
}

int lqmpc_max_vn_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int K, const double *A, const double *B,
                       const double *Q, const double *R, const double *P, const double *lb, const double *ub,
                       const double *x0s, const double *x_ref, const double *u_ref, double *MV, int32_t *status,
                       int32_t *iters)
{
    if (!h || !A || !B || !x0s || !MV) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB;
    double *dMV;
    int32_t *dst, *dit;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB);
    s.out(MV, b, dMV); s.out(status, b, dst); s.out(iters, b, dit);
    rc = s.upload();
    if (!rc) rc = lqmpc_max_vn_batch_dev(h, nx, nu, N, Bsz, K, dA, dB, Q, R, P, lb, ub, x0s, x_ref, u_ref, dMV, dst, dit);
    return rc ? rc : s.finish();
}

int lqmpc_sweep_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, int K, const double *A, const double *B,
                      const double *Q, const double *R, const double *P, const double *lb, const double *ub, const double *x0,
                      const double *x0s, const double *A_true, const double *B_true, int true_per_instance, const double *x_ref,
                      const double *u_ref, double *JT, double *MV, int32_t *status, int32_t *iters)
{
    if (!h || !A || !B || !x0 || !x0s || !JT || !MV || !A_true || !B_true) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *dx0, *dAt = A_true, *dBt = B_true;
    double *dJT, *dMV;
    int32_t *dst, *dit;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(x0, b * nx, dx0);
    if (true_per_instance) { s.in(A_true, b * nx * nx, dAt); s.in(B_true, b * nx * nu, dBt); }
    s.out(JT, b, dJT); s.out(MV, b, dMV); s.out(status, b, dst); s.out(iters, b, dit);
    rc = s.upload();
    if (!rc) rc = lqmpc_sweep_batch_dev(h, nx, nu, N, Bsz, T, K, dA, dB, Q, R, P, lb, ub, dx0, x0s, dAt, dBt, true_per_instance, x_ref,
                                        u_ref, dJT, dMV, dst, dit);
    return rc ? rc : s.finish();
}

// ---- the bound coefficients of data_generation: lqmpc_bounds.hip ----
int lqmpc_bounds_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB,
                           const double *Q, const double *R, const double *lb, const double *ub, const double *de_A,
                           const double *de_B, const double *dMV, const double *x, const double *p3, double V_expert,
                           double *dK, double *dalpha, double *dbeta, double *dxi, double *deta, double *dbound, double *deps,
                           double *daux, int32_t *dstatus)
{
    if (!h || !dA || !dB || !Q || !R || !lb || !ub || !de_A || !de_B || !x || !p3) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    for (int k = 0; k < nu; ++k)
        if (!(ub[k] > lb[k]) || !std::isfinite(lb[k]) || !std::isfinite(ub[k]) || lb[k] == 0.0 || ub[k] == 0.0)
            return fail(LQMPC_ERR_BAD_ARG, "every input needs a finite box with lb < ub and non-zero bounds (rows of F_u)");
    for (int k = 0; k < 3; ++k)
        if (!(p3[k] > 0.0)) return fail(LQMPC_ERR_BAD_ARG, "p must be positive");
    HIP_TRY(hipSetDevice(h->device));
    // batch-shared block: Q | R | Q^-1 | R^-1 | lb | ub | x | p | (qmax qmin rmax rmin V_expert bar_u bar_d_u)
    std::vector<double> sh;
    auto put = [&](const double *src, int count) { int off = (int)sh.size(); sh.insert(sh.end(), src, src + count); return off; };
    lqmpc::BoundsParams bp;
    memset(&bp, 0, sizeof bp);
    bp.oQ = put(Q, nx * nx); bp.oR = put(R, nu * nu);
    std::vector<double> Qi(Q, Q + nx * nx), Ri(R, R + nu * nu);
    double qmax, qmin, rmax, rmin;
    if (!host_sym_eig_extremes(Q, nx, qmax, qmin) || !host_sym_eig_extremes(R, nu, rmax, rmin) || !(qmin > 0.0) || !(rmin > 0.0) ||
        !host_spd_inverse(Qi, nx) || !host_spd_inverse(Ri, nu))
        return fail(LQMPC_ERR_BAD_ARG, "Q and R must be symmetric positive definite");
    bp.oQinv = put(Qi.data(), nx * nx); bp.oRinv = put(Ri.data(), nu * nu);
    bp.olb = put(lb, nu); bp.oub = put(ub, nu); bp.ox = put(x, nx); bp.op = put(p3, 3);
    double bar_u = 0.0, bar_du = 0.0;                    // max |u|^2 and max |u1 - u2|^2 over the box (utils.py:592-650 solves two QPs for these)
    for (int k = 0; k < nu; ++k) { bar_u += std::max(lb[k] * lb[k], ub[k] * ub[k]); bar_du += (ub[k] - lb[k]) * (ub[k] - lb[k]); }
    const double sc[7] = {qmax, qmin, rmax, rmin, V_expert, bar_u, bar_du};
    bp.osc = put(sc, 7);
    // for the on-chip kernels: identity / zero weights (Gamma'Gamma is the condensed Hessian with them), and whether Q, R are multiples of I
    std::vector<double> eye((size_t)nx * nx, 0.0), zer((size_t)nu * nu, 0.0);
    for (int a = 0; a < nx; ++a) eye[(size_t)a * nx + a] = 1.0;
    bp.oI = put(eye.data(), nx * nx); bp.oZ = put(zer.data(), nu * nu);
    auto scalar_mult = [](const double *M, int n) { for (int a = 0; a < n; ++a) for (int c = 0; c < n; ++c) if (M[a * n + c] != (a == c ? M[0] : 0.0)) return false; return true; };
    bp.q_scalar = scalar_mult(Q, nx) ? 1 : 0; bp.r_scalar = scalar_mult(R, nu) ? 1 : 0;
    bp.qs = Q[0]; bp.rs = R[0];
    rc = ensure(h, h->shared, std::max(sh.size(), (size_t)8192) * sizeof(double));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h->shared.p, sh.data(), sh.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->shared_host.clear();                              // the solver's cached copy of the shared block is gone
    bp.o = lqmpc::bounds_offsets(nx, nu, N);
    bp.nx = nx; bp.nu = nu; bp.N = N; bp.Bsz = Bsz;
    bp.A = dA; bp.B = dB; bp.eA = de_A; bp.eB = de_B; bp.MV = dMV; bp.sh = (const double *)h->shared.p;
    bp.K = dK; bp.alpha = dalpha; bp.beta = dbeta; bp.xi = dxi; bp.eta = deta; bp.bound = dbound; bp.eps = deps; bp.aux = daux;
    bp.status = dstatus;
    // the on-chip kernels (registers + LDS, two launches): prebuilt for the reference's shapes, compiled at run time for the others;
    // the HBM-workspace kernel below stays for what neither serves (kernel = generic forces it)
    if (h->opt.kernel != LQMPC_KERNEL_GENERIC) {
        rc = ensure(h, h->ws, (size_t)Bsz * 10 * sizeof(double));
        if (rc) return rc;
        bp.rec = (double *)h->ws.p; bp.b0 = 0; bp.b1 = Bsz;
        bool done = lqmpc::launch_bounds_chip(bp, h->stream);
        if (!done && h->opt.jit != 0) {
            std::string why;
            done = lqmpc::launch_jit_bounds(h->device, bp, h->stream, &why);
            if (!done) g_err = "on-chip bounds kernels unavailable, using the workspace kernel: " + why;
        }
        if (done) {
            HIP_TRY(hipGetLastError());
            set_last_kernel(h, "lqmpc_bounds_small_kernel + lqmpc_bounds_big_kernel");
            return 0;
        }
    }
    // workspace: at most ~1 GiB at a time, the batch in chunks of whole wavefronts
    const size_t per = (size_t)bp.o.total * sizeof(double);
    long long chunk = (long long)(((size_t)1 << 30) / per) / 64 * 64;
    if (chunk < 64) chunk = 64;
    if (chunk > (Bsz + 63) / 64 * 64) chunk = (Bsz + 63) / 64 * 64;
    rc = ensure(h, h->ws, per * (size_t)chunk);
    if (rc) return rc;
    bp.ws = (double *)h->ws.p; bp.stride = chunk;
    for (long long b0 = 0; b0 < Bsz; b0 += chunk) {
        bp.b0 = b0; bp.b1 = std::min<long long>(Bsz, b0 + chunk);
        lqmpc::launch_bounds(bp, h->stream);
        HIP_TRY(hipGetLastError());
    }
    set_last_kernel(h, "lqmpc_bounds_kernel");
    return 0;
}

int lqmpc_bounds_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B,
                       const double *Q, const double *R, const double *lb, const double *ub, const double *e_A,
                       const double *e_B, const double *MV, const double *x, const double *p3, double V_expert,
                       double *K, double *alpha, double *beta, double *xi, double *eta, double *bound, double *eps,
                       double *aux, int32_t *status)
{
    if (!h || !A || !B || !e_A || !e_B) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = check_dims(nx, nu, N, Bsz);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    s.may_pack = false;                                  // (as this entry point always has: its copies are not the cost of a call)
    const size_t b = (size_t)Bsz;
    const double *dA, *dB, *deA, *deB, *dMV;
    double *dK, *dal, *dbe, *dxi, *det, *dbd, *dep, *dax;
    int32_t *dst;
    s.in(A, b * nx * nx, dA); s.in(B, b * nx * nu, dB); s.in(e_A, b, deA); s.in(e_B, b, deB); s.in(MV, b, dMV);
    s.out(K, b * nu * nx, dK); s.out(alpha, b, dal); s.out(beta, b, dbe); s.out(xi, b, dxi); s.out(eta, b, det);
    s.out(bound, b, dbd); s.out(eps, b, dep); s.out(aux, b * 8, dax); s.out(status, b, dst);
    rc = s.upload();
    if (!rc) rc = lqmpc_bounds_batch_dev(h, nx, nu, N, Bsz, dA, dB, Q, R, lb, ub, deA, deB, dMV, x, p3, V_expert, dK, dal, dbe, dxi, det, dbd,
                                         dep, dax, dst);
    return rc ? rc : s.finish();
}

int lqmpc_timer_begin(lqmpc_handle *h)
{
    if (!h) return fail(LQMPC_ERR_BAD_ARG, "handle is NULL");
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    return 0;
}

int lqmpc_timer_end(lqmpc_handle *h, float *ms)
{
    if (!h || !ms) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipEventSynchronize(h->ev1));
    HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Prepared controllers: the per-instance set-up kept in HBM, one QP per instance and call from it (kernels: lqmpc_ctl.hip).
struct lqmpc_controller {
    lqmpc_handle *h = nullptr;
    uint64_t id = 0;                          // what the handle remembers of the controller that set last_kernel
    lqmpc_options opt;                        // the handle's options when the controller was made: every step is planned and filled from these
    int nx = 0, nu = 0, N = 0;
    int64_t Bsz = 0;
    std::vector<double> Q, R, P, lb, ub, xref, uref;
    bool has_xref = false, has_uref = false;
    void *A = nullptr, *B = nullptr;          // the controller's copies (instance-minor): the hand-back and the pass-through read them
    void *rec = nullptr, *face = nullptr;     // fast path: records (CtlRec); per instance the previous face, its state, the expected next state
    void *vn = nullptr;                       // V_N of a step whose caller passed NULL (the solve kernels always write it); on first need
    size_t bytes = 0;
    bool fast = false, jit = false;           // fast: the record kernels serve the shape (jit: compiled at run time); else pass-through
    bool wg = false;                          // fast, on the workgroup kernel's shapes (options.ctl_wg): one launch per step, no hand-back
    std::string name = "lqmpc_solve_batch_dev";
    std::string roll_name;                    // fast: the record kernel of lqmpc_controller_rollout
    int roll_jit = -1;                        // jit: whether that kernel could be had (-1: not asked yet; 0: the rollout passes through)
};

namespace {

void ctl_free(lqmpc_controller *c)
{
    for (void *q : {c->A, c->B, c->rec, c->face, c->vn}) if (q) (void)hipFree(q);
    delete c;
}

int ctl_alloc(lqmpc_controller *c, void **q, size_t bytes)
{
    const hipError_t e = hipMalloc(q, bytes);
    if (e != hipSuccess) { *q = nullptr; return fail(LQMPC_ERR_ALLOC, std::string("hipMalloc (controller): ") + hipGetErrorString(e)); }
    c->bytes += bytes;
    return 0;
}

Call ctl_call(const lqmpc_controller *c)
{
    return Call{c->nx, c->nu, c->N, 0, 0, lqmpc::MODE_SOLVE, 0, c->Bsz, c->Q.data(), c->R.data(), c->P.data(), c->lb.data(), c->ub.data(),
                c->has_xref ? c->xref.data() : nullptr, c->has_uref ? c->uref.data() : nullptr, nullptr, nullptr, nullptr};
}

int ctl_launch(lqmpc_controller *c, const KParams &p)
{
    lqmpc_handle *h = c->h;
    if (c->jit) {
        std::string why;
        if (!lqmpc::launch_jit(h->device, p, h->stream, nullptr, &why)) return fail(LQMPC_ERR_HIP, "run-time compiled controller kernel: " + why);
    } else if (c->wg) {
        if (!lqmpc::launch_wg_ctl(p, h->stream, nullptr)) return fail(LQMPC_ERR_HIP, "workgroup controller kernel launch failed");
    } else if (!lqmpc::launch_ctl(p, h->stream, nullptr)) return fail(LQMPC_ERR_UNSUPPORTED, "controller kernel launch failed");
    HIP_TRY(hipGetLastError());
    return 0;
}

// per instance: the words of its face entry, the doubles of its record
struct CtlSizes { size_t face_words, stride; };
CtlSizes ctl_sizes(const lqmpc_controller *c)
{
    if (c->wg) return {(size_t)(lqmpc::WG_CTL_FACE_WORDS + 2 * c->nx), (size_t)lqmpc::wg_ctl_rec_layout(c->nx, c->nu, c->N).stride};
    return {(size_t)(2 + 2 * c->nx), (size_t)lqmpc::ctl_rec_layout(c->nx, c->nu, c->N).stride};
}

void ctl_bind(const lqmpc_controller *c, KParams &p)
{
    p.A = (const double *)c->A; p.B = (const double *)c->B;
    p.ctl_rec = (double *)c->rec;
    p.ctl_stride = (long long)ctl_sizes(c).stride;
    p.ctl_face = (unsigned long long *)c->face;
    p.ctl_idx = nullptr; p.ctl_n = c->Bsz;
}

// the argument checks, the shared block and the plan of `cl` on the controller's handle under its option snapshot, as at create and
// at every step; the parameter block bound to its records and copies
int ctl_prepare(const lqmpc_controller *c, const Call &cl, KParams &p, Plan &pl)
{
    const int rc = prepare(c->h, c->opt, cl, p, pl);
    if (!rc) ctl_bind(c, p);
    return rc;
}

// V_N of a step whose caller passed NULL: allocated on first need
int ctl_vn(lqmpc_controller *c) { return c->vn ? 0 : ctl_alloc(c, &c->vn, (size_t)c->Bsz * sizeof(double)); }

// One record-path call with `p` filled: the launch on the records, then whatever it handed back -- the instances that did not settle
// within r16_maxit iterations or met a non-finite state -- from scratch in mode `hand_back` on the existing kernels, over the
// device-side list and from the controller's copies of A and B, as launch_rows does for a one-shot call.  The workgroup records hand
// nothing back: their fall-back (interior point on the n x n matrices) is inside solve_qp, one launch.
int ctl_run(lqmpc_controller *c, const Plan &pl, KParams &p, int hand_back, bool need_vn, const std::string &name)
{
    lqmpc_handle *h = c->h;
    const bool list = !c->wg;
    int rc = list ? prepare_hand_back(h, p) : 0;
    if (!rc) rc = ctl_launch(c, p);
    if (!rc && list && need_vn) rc = ctl_vn(c);
    if (!rc && list) rc = launch_hand_back(h, pl, p, hand_back, need_vn ? (double *)c->vn : nullptr);
    if (!rc) set_last_kernel(h, name.c_str(), c->id);
    return rc;
}

int ctl_create(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B, hipMemcpyKind kind, const double *Q,
               const double *R, const double *P, const double *lb, const double *ub, const double *x_ref, const double *u_ref,
               lqmpc_controller **out)
{
    if (out) *out = nullptr;
    if (!h || !out || !A || !B) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    // the argument checks, the shared block and the plan of an ordinary solve on this handle
    Call c0{nx, nu, N, 0, 0, lqmpc::MODE_SOLVE, 0, Bsz, Q, R, P, lb, ub, x_ref, u_ref, nullptr, nullptr, nullptr};
    KParams p;
    Plan pl;
    int rc = prepare(h, h->opt, c0, p, pl);
    if (rc) return rc;
    lqmpc_controller *c = new lqmpc_controller();
    c->h = h; c->id = ++h->ctl_ids; c->opt = h->opt; c->nx = nx; c->nu = nu; c->N = N; c->Bsz = Bsz;
    c->Q.assign(Q, Q + nx * nx); c->R.assign(R, R + nu * nu); c->P.assign(P, P + nx * nx);
    c->lb.assign(lb, lb + nu); c->ub.assign(ub, ub + nu);
    if (x_ref) { c->xref.assign(x_ref, x_ref + nx * N); c->has_xref = true; }
    if (u_ref) { c->uref.assign(u_ref, u_ref + nu * N); c->has_uref = true; }
    // fast path: where that plan runs the 16-lane-row family
    if (pl.rows()) {
        if (pl.family == FAM_R16 && lqmpc::ctl_available(nx, nu, N)) c->fast = true;
        else if (h->opt.jit != 0) {
            std::string why;
            c->fast = c->jit = lqmpc::jit_available(h->device, nx, nu, N, lqmpc::MODE_CTL_FACTOR, &why) &&
                               lqmpc::jit_available(h->device, nx, nu, N, lqmpc::MODE_CTL_STEP, &why);
            if (!c->fast) g_err = "run-time compile unavailable, the controller passes through to lqmpc_solve_batch_dev: " + why;
        }
    } else if (h->opt.ctl_wg == 1 && pl.family == FAM_WG && p.presolve && p.warm_start) {
        // opt-in (a record is two images of the block triangle: 166 KB per instance at (8,4,30)): records on the workgroup kernel's shapes
        c->fast = c->wg = true;
    }
    const size_t face_words = ctl_sizes(c).face_words, rec_doubles = ctl_sizes(c).stride;
    const size_t b = (size_t)Bsz, nA = b * nx * nx * sizeof(double), nB = b * nx * nu * sizeof(double);
    rc = ctl_alloc(c, &c->A, nA);
    if (!rc) rc = ctl_alloc(c, &c->B, nB);
    if (!rc && c->fast) {
        rc = ctl_alloc(c, &c->rec, b * rec_doubles * sizeof(double));
        if (!rc) rc = ctl_alloc(c, &c->face, b * face_words * sizeof(unsigned long long));
    }
    if (rc) { ctl_free(c); return rc; }
    hipError_t e = hipMemcpyAsync(c->A, A, nA, kind, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->B, B, nB, kind, h->stream);
    if (e == hipSuccess && c->fast) e = hipMemsetAsync(c->face, 0, b * face_words * sizeof(unsigned long long), h->stream);
    if (e != hipSuccess) { ctl_free(c); return fail(LQMPC_ERR_HIP, std::string("controller copy: ") + hipGetErrorString(e)); }
    if (c->fast) {
        char nm[96];
        snprintf(nm, sizeof nm, "lqmpc_ctl_r%d%s_kernel<%d,%d,%d>", N * nu <= 32 ? 16 : 64, c->jit ? "_jit" : "", nx, nu, N);
        if (!c->jit && lqmpc::r16_lanes(nx, nu, N) == 64) snprintf(nm, sizeof nm, "lqmpc_ctl_r64_kernel<%d,%d,%d>", nx, nu, N);
        c->name = c->wg ? "lqmpc_wg_ctl_step_kernel" : nm;
        snprintf(nm, sizeof nm, "lqmpc_ctl_roll_r%d%s_kernel<%d,%d,%d>", lqmpc::r16_lanes(nx, nu, N) == 64 || N * nu > 32 ? 64 : 16,
                 c->jit ? "_jit" : "", nx, nu, N);
        c->roll_name = c->wg ? "lqmpc_wg_ctl_rollout_kernel" : nm;
        ctl_bind(c, p);
        p.mode = lqmpc::MODE_CTL_FACTOR;
        rc = ctl_launch(c, p);
        if (rc) { ctl_free(c); return rc; }
    }
    // the caller may overwrite A and B as soon as this returns
    e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { ctl_free(c); return fail(LQMPC_ERR_HIP, std::string("controller set-up: ") + hipGetErrorString(e)); }
    if (c->wg) {
        // the records hold A and B, and nothing is handed back to a kernel that would read the copies
        (void)hipFree(c->A); (void)hipFree(c->B);
        c->A = c->B = nullptr;
        c->bytes -= nA + nB;
    }
    *out = c;
    return 0;
}

}  // namespace

extern "C" {

int lqmpc_controller_create(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B, const double *Q,
                            const double *R, const double *P, const double *lb, const double *ub, const double *x_ref,
                            const double *u_ref, lqmpc_controller **out)
{
    return ctl_create(h, nx, nu, N, Bsz, A, B, hipMemcpyHostToDevice, Q, R, P, lb, ub, x_ref, u_ref, out);
}

int lqmpc_controller_create_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB, const double *Q,
                                const double *R, const double *P, const double *lb, const double *ub, const double *x_ref,
                                const double *u_ref, lqmpc_controller **out)
{
    return ctl_create(h, nx, nu, N, Bsz, dA, dB, hipMemcpyDeviceToDevice, Q, R, P, lb, ub, x_ref, u_ref, out);
}

}  // extern "C"

// lqmpc_controller_step_dev, and with dUplan (dXplan may be null) lqmpc_controller_step_plan_dev
static int ctl_step_dev(lqmpc_controller *c, const double *dx, double *du0, double *dVN, double *dUplan, double *dXplan, int32_t *dstatus,
                        int32_t *diters, lqmpc::SharedOff *so = nullptr)
{
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    const Call cl = ctl_call(c);
    if (!c->fast) {
        // pass-through: the existing solve path, unchanged, on the controller's copies of A and B
        int rc = dVN ? 0 : ctl_vn(c);
        if (!rc) rc = solve_dev(h, c->opt, cl, (const double *)c->A, (const double *)c->B, dx, du0, dVN ? dVN : (double *)c->vn, dstatus, diters,
                                dUplan, dXplan, so);
        if (!rc) c->name = h->last_kernel;
        return rc;
    }
    KParams p;
    Plan pl;
    int rc = ctl_prepare(c, cl, p, pl);
    if (rc) return rc;
    if (so) *so = p.so;
    p.x0 = dx; p.u0 = du0; p.VN = dVN; p.status = dstatus; p.iters = diters;
    p.Uplan = dUplan; p.Xplan = dXplan;
    p.mode = lqmpc::MODE_CTL_STEP;
    return ctl_run(c, pl, p, lqmpc::MODE_SOLVE, !dVN, c->name);
}

extern "C" {

int lqmpc_controller_step_dev(lqmpc_controller *c, const double *dx, double *du0, double *dVN, int32_t *dstatus, int32_t *diters)
{
    if (!c || !dx || !du0) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    return ctl_step_dev(c, dx, du0, dVN, nullptr, nullptr, dstatus, diters);
}

int lqmpc_controller_step_plan_dev(lqmpc_controller *c, const double *dx, double *du0, double *dVN, double *dUplan, double *dXplan,
                                   int32_t *dstatus, int32_t *diters)
{
    if (!c || !dx || !du0 || !dUplan) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    return ctl_step_dev(c, dx, du0, dVN, dUplan, dXplan, dstatus, diters);
}

int lqmpc_controller_step_plan(lqmpc_controller *c, const double *x, double *u0, double *VN, double *Uplan, double *Xplan, int32_t *status,
                               int32_t *iters)
{
    if (!c || !x || !u0 || !Uplan) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)c->Bsz;
    const double *dx;
    double *du0, *dVN, *dUp, *dXp;
    int32_t *dst, *dit;
    s.in(x, b * c->nx, dx);
    s.out(u0, b * c->nu, du0); s.out(VN, b, dVN); s.out(Uplan, b * c->nu * c->N, dUp); s.out(Xplan, b * c->nx * (c->N + 1), dXp);
    s.out(status, b, dst); s.out(iters, b, dit);
    int rc = s.upload();
    if (!rc) rc = lqmpc_controller_step_plan_dev(c, dx, du0, dVN, dUp, dXp, dst, dit);
    return rc ? rc : s.finish();
}

int lqmpc_controller_step_sens_dev(lqmpc_controller *c, const double *dx, double *du0, double *dVN, double *dK0, double *ddVdx,
                                   double *dKplan, double *dUplan, double *dXplan, int32_t *dstatus, int32_t *diters)
{
    if (!c || !dx || !du0 || !dK0 || !ddVdx) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    int rc = sens_buffers(h, c->nx, c->nu, c->N, c->Bsz, dUplan, dXplan, dstatus);
    if (rc) return rc;
    // the model of every instance: the controller's instance-minor copies, or (workgroup records keep none) the heads of its records
    lqmpc::SensParams s{c->nx, c->nu, c->N, c->Bsz, (const double *)c->A, (const double *)c->B, c->Bsz, 1, dUplan, dXplan, dstatus,
                        nullptr, {}, dK0, ddVdx, dKplan};
    if (!c->A) {
        const lqmpc::WgCtlRec L = lqmpc::wg_ctl_rec_layout(c->nx, c->nu, c->N);
        s.A = (const double *)c->rec + L.oA; s.B = (const double *)c->rec + L.oB;
        s.sE = 1; s.sI = L.stride;
    }
    rc = ctl_step_dev(c, dx, du0, dVN, dUplan, dXplan, dstatus, diters, &s.so);
    return rc ? rc : sens_launch(h, s);
}

int lqmpc_controller_step_sens(lqmpc_controller *c, const double *x, double *u0, double *VN, double *K0, double *dVdx, double *Kplan,
                               double *Uplan, double *Xplan, int32_t *status, int32_t *iters)
{
    if (!c || !x || !u0 || !K0 || !dVdx) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)c->Bsz, nx = (size_t)c->nx, nu = (size_t)c->nu, N = (size_t)c->N;
    const double *dx;
    double *du0, *dVN, *dK0, *ddV, *dKp, *dUp, *dXp;
    int32_t *dst, *dit;
    s.in(x, b * nx, dx);
    s.out(u0, b * nu, du0); s.out(VN, b, dVN); s.out(K0, b * nu * nx, dK0); s.out(dVdx, b * nx, ddV);
    s.out(Kplan, b * nu * N * nx, dKp); s.out(Uplan, b * nu * N, dUp); s.out(Xplan, b * nx * (N + 1), dXp);
    s.out(status, b, dst); s.out(iters, b, dit);
    int rc = s.upload();
    if (!rc) rc = lqmpc_controller_step_sens_dev(c, dx, du0, dVN, dK0, ddV, dKp, dUp, dXp, dst, dit);
    return rc ? rc : s.finish();
}

// read-only on the controller: its copies of A and B (on workgroup records the heads of the records) and its current references
int lqmpc_controller_model_grad_dev(lqmpc_controller *c, const double *dUplan, const double *dXplan, const int32_t *dstatus,
                                    const double *dgu0, const double *dgVN, double *dgA, double *dgB, double *dgx0)
{
    int rc = grad_check(c, nullptr, dUplan, dXplan, dgu0, dgVN, dgA, dgB);
    if (rc) return rc;
    lqmpc::GradParams g{c->nx, c->nu, c->N, c->Bsz, (const double *)c->A, (const double *)c->B, c->Bsz, 1, dUplan, dXplan, dstatus,
                        nullptr, {}, dgu0, dgVN, dgA, dgB, dgx0};
    if (!c->A) {
        const lqmpc::WgCtlRec L = lqmpc::wg_ctl_rec_layout(c->nx, c->nu, c->N);
        g.A = (const double *)c->rec + L.oA; g.B = (const double *)c->rec + L.oB;
        g.sE = 1; g.sI = L.stride;
    }
    return grad_launch(c->h, ctl_call(c), g);
}

int lqmpc_controller_model_grad(lqmpc_controller *c, const double *Uplan, const double *Xplan, const int32_t *status,
                                const double *gu0, const double *gVN, double *gA, double *gB, double *gx0)
{
    int rc = grad_check(c, nullptr, Uplan, Xplan, gu0, gVN, gA, gB);
    if (rc) return rc;
    if (!lqmpc::grad_fits(c->nx, c->nu, c->N)) return fail(LQMPC_ERR_UNSUPPORTED, "lqmpc_grad_kernel: the LDS image of this shape is over 160 KiB");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)c->Bsz, nx = (size_t)c->nx, nu = (size_t)c->nu, N = (size_t)c->N;
    const double *dUp, *dXp, *dgu, *dgV;
    const int32_t *dst;
    double *dgA, *dgB, *dgx;
    s.in(Uplan, b * nu * N, dUp); s.in(Xplan, b * nx * (N + 1), dXp); s.in(status, b, dst); s.in(gu0, b * nu, dgu); s.in(gVN, b, dgV);
    s.out(gA, b * nx * nx, dgA); s.out(gB, b * nx * nu, dgB); s.out(gx0, b * nx, dgx);
    rc = s.upload();
    if (!rc) rc = lqmpc_controller_model_grad_dev(c, dUp, dXp, dst, dgu, dgV, dgA, dgB, dgx);
    return rc ? rc : s.finish();
}

// read-only on the controller: its copies of A and B (on workgroup records the heads of the records) and its current references
int lqmpc_controller_plan_grad_dev(lqmpc_controller *c, const double *dUplan, const double *dXplan, const int32_t *dstatus,
                                   const double *dgUplan, const double *dgXplan, const double *dgVN, double *dgA, double *dgB, double *dgx0)
{
    if (!c) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    lqmpc::PGradParams g{c->nx, c->nu, c->N, c->Bsz, (const double *)c->A, (const double *)c->B, c->Bsz, 1, dUplan, dXplan, dstatus,
                         nullptr, {}, dgUplan, dgXplan, dgVN, dgA, dgB, dgx0};
    if (!c->A) {
        const lqmpc::WgCtlRec L = lqmpc::wg_ctl_rec_layout(c->nx, c->nu, c->N);
        g.A = (const double *)c->rec + L.oA; g.B = (const double *)c->rec + L.oB;
        g.sE = 1; g.sI = L.stride;
    }
    return pgrad_launch(c->h, nullptr, ctl_call(c), g);
}

int lqmpc_controller_plan_grad(lqmpc_controller *c, const double *Uplan, const double *Xplan, const int32_t *status,
                               const double *gUplan, const double *gXplan, const double *gVN, double *gA, double *gB, double *gx0)
{
    if (!c) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    int rc = pgrad_check(c, nullptr, c->nx, c->nu, c->N, Uplan, Xplan, gUplan, gXplan, gVN, gA, gB, gx0);
    if (rc) return rc;
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)c->Bsz, nx = (size_t)c->nx, nu = (size_t)c->nu, N = (size_t)c->N;
    const double *dUp, *dXp, *dgU, *dgX, *dgV;
    const int32_t *dst;
    double *dgA, *dgB, *dgx;
    s.in(Uplan, b * nu * N, dUp); s.in(Xplan, b * nx * (N + 1), dXp); s.in(status, b, dst);
    s.in(gUplan, b * nu * N, dgU); s.in(gXplan, b * nx * (N + 1), dgX); s.in(gVN, b, dgV);
    s.out(gA, b * nx * nx, dgA); s.out(gB, b * nx * nu, dgB); s.out(gx0, b * nx, dgx);
    rc = s.upload();
    if (!rc) rc = lqmpc_controller_plan_grad_dev(c, dUp, dXp, dst, dgU, dgX, dgV, dgA, dgB, dgx);
    return rc ? rc : s.finish();
}

// read-only on the controller: its copies of A and B (on workgroup records the heads of the records) and its current references
int lqmpc_controller_cost_grad_dev(lqmpc_controller *c, const double *dUplan, const double *dXplan, const int32_t *dstatus,
                                   const double *dgu0, const double *dgVN, int reduce, double *dgQ, double *dgR, double *dgP, double *dglb,
                                   double *dgub, double *dgxref, double *dguref, int64_t *dnskipped)
{
    double *const outs[7] = {dgQ, dgR, dgP, dglb, dgub, dgxref, dguref};
    const int rc = cgrad_nulls(c, dUplan, dXplan, dgu0, dgVN, outs);
    if (rc) return rc;
    lqmpc::CGradParams g{c->nx, c->nu, c->N, c->Bsz, (const double *)c->A, (const double *)c->B, c->Bsz, 1, dUplan, dXplan, dstatus,
                         nullptr, {}, dgu0, dgVN, reduce ? 1 : 0, {dgQ, dgR, dgP, dglb, dgub, dgxref, dguref}, (long long *)dnskipped, nullptr};
    if (!c->A) {
        const lqmpc::WgCtlRec L = lqmpc::wg_ctl_rec_layout(c->nx, c->nu, c->N);
        g.A = (const double *)c->rec + L.oA; g.B = (const double *)c->rec + L.oB;
        g.sE = 1; g.sI = L.stride;
    }
    return cgrad_launch(c->h, ctl_call(c), g);
}

int lqmpc_controller_cost_grad(lqmpc_controller *c, const double *Uplan, const double *Xplan, const int32_t *status,
                               const double *gu0, const double *gVN, int reduce, double *gQ, double *gR, double *gP, double *glb,
                               double *gub, double *gxref, double *guref, int64_t *nskipped)
{
    double *const outs[7] = {gQ, gR, gP, glb, gub, gxref, guref};
    int rc = cgrad_nulls(c, Uplan, Xplan, gu0, gVN, outs);
    if (rc) return rc;
    rc = cgrad_check(c, nullptr, c->nx, c->nu, c->N, Uplan, Xplan, gu0, gVN, reduce, outs);
    if (rc) return rc;
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)c->Bsz, nx = (size_t)c->nx, nu = (size_t)c->nu, N = (size_t)c->N, per = reduce ? 1 : b;
    size_t n[7];
    cgrad_counts(c->nx, c->nu, c->N, n);
    const double *dUp, *dXp, *dgu, *dgV;
    const int32_t *dst;
    double *d[7];
    int64_t *dns;
    s.in(Uplan, b * nu * N, dUp); s.in(Xplan, b * nx * (N + 1), dXp); s.in(status, b, dst); s.in(gu0, b * nu, dgu); s.in(gVN, b, dgV);
    for (int k = 0; k < 7; ++k) s.out(outs[k], n[k] * per, d[k]);
    s.out(reduce ? nskipped : (int64_t *)nullptr, 1, dns);
    rc = s.upload();
    if (!rc) rc = lqmpc_controller_cost_grad_dev(c, dUp, dXp, dst, dgu, dgV, reduce, d[0], d[1], d[2], d[3], d[4], d[5], d[6], dns);
    return rc ? rc : s.finish();
}

int lqmpc_controller_step(lqmpc_controller *c, const double *x, double *u0, double *VN, int32_t *status, int32_t *iters)
{
    if (!c || !x || !u0) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)c->Bsz;
    const double *dx;
    double *du0, *dVN;
    int32_t *dst, *dit;
    s.in(x, b * c->nx, dx);
    s.out(u0, b * c->nu, du0); s.out(VN, b, dVN); s.out(status, b, dst); s.out(iters, b, dit);
    int rc = s.upload();
    if (!rc) rc = lqmpc_controller_step_dev(c, dx, du0, dVN, dst, dit);
    return rc ? rc : s.finish();
}

// T closed-loop steps of every instance from the controller's present state, in one launch.  Read-only on the controller: the
// rollout starts cold and carries its own face inside the kernel; ctl_face and the records are not written.
//
// Routing of a 16-lane-row record controller (the workgroup records have one kernel, 10.9 against 13.5 ms at C5 x 32 768, and no
// copies of A, B to pass through with).  Measured on one MI355X, T = 30, default mix, record kernel against lqmpc_rollout_batch_dev
// (profiles/controller_rollout.json, "record kernel at every size"): C3 0.176 against 0.170 ms at 4 096 instances, 0.196 / 0.218 at
// 8 192, 0.228 / 0.217 at 16 384, 0.317 / 0.230 at 32 768, 0.488 / 0.305 at 65 536; C4 x 262 144 6.02 against 4.18 ms.  The record
// kernel walks the batch in natural order without the set-up's cold-start guess; the one-shot call orders by difficulty from 8 192
// instances (make_plan) and gains more from that than its set-up costs.  From the smallest size measured, 4 096, the record kernel is
// not faster by more than the +-3 % of lease noise, so from there the rollout goes to lqmpc_rollout_batch_dev on the controller's
// copies; below it (not measured against the one-shot call: a handful of wavefronts, where the set-up is latency on the only
// wavefront a SIMD has) it stays on the records.
constexpr int64_t CTL_ROLL_ROWS_MAX = 4095;
int lqmpc_controller_rollout_dev(lqmpc_controller *c, int T, const double *dx0, const double *A_true, const double *B_true,
                                 int true_per_instance, double *dJT, double *dX, double *dU, int32_t *dstatus, int32_t *diters)
{
    if (!c || !dx0 || !A_true || !B_true || !dJT) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    const int tpi = true_per_instance ? 1 : 0;
    Call cl = ctl_call(c);
    cl.T = T; cl.true_per_instance = tpi; cl.At_sh = A_true; cl.Bt_sh = B_true;
    bool rec = c->fast && (c->wg || c->Bsz <= CTL_ROLL_ROWS_MAX);
    if (rec && c->jit) {
        if (c->roll_jit < 0) {
            std::string why;
            c->roll_jit = lqmpc::jit_available(h->device, c->nx, c->nu, c->N, lqmpc::MODE_CTL_ROLL, &why) ? 1 : 0;
            if (!c->roll_jit) g_err = "run-time compile unavailable, the controller's rollout passes through to lqmpc_rollout_batch_dev: " + why;
        }
        rec = c->roll_jit == 1;
    }
    if (!rec) {
        // pass-through: the one-shot rollout under the controller's option snapshot, on its copies of A and B, with its references
        cl.mode = lqmpc::MODE_ROLLOUT;
        return rollout_dev(h, c->opt, cl, (const double *)c->A, (const double *)c->B, dx0, A_true, B_true, dJT, dX, dU, dstatus, diters);
    }
    // planned as a step is (the family of create, no order); the shared block carries a shared plant
    KParams p;
    Plan pl;
    int rc = ctl_prepare(c, cl, p, pl);
    if (rc) return rc;
    p.ctl_face = nullptr;
    p.x0 = dx0; p.JT = dJT; p.X = dX; p.U = dU; p.status = dstatus; p.iters = diters;
    if (tpi) { p.At = A_true; p.Bt = B_true; }
    p.mode = lqmpc::MODE_CTL_ROLL;
    // (a handed-back instance runs its whole rollout again)
    return ctl_run(c, pl, p, lqmpc::MODE_ROLLOUT, false, c->roll_name);
}

int lqmpc_controller_rollout(lqmpc_controller *c, int T, const double *x0, const double *A_true, const double *B_true,
                             int true_per_instance, double *JT, double *X, double *U, int32_t *status, int32_t *iters)
{
    if (!c || !x0 || !A_true || !B_true || !JT) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)c->Bsz, nx = (size_t)c->nx, nu = (size_t)c->nu;
    const double *dx0, *dAt = A_true, *dBt = B_true;
    double *dJT, *dX, *dU;
    int32_t *dst, *dit;
    s.in(x0, b * nx, dx0);
    if (true_per_instance) { s.in(A_true, b * nx * nx, dAt); s.in(B_true, b * nx * nu, dBt); }
    s.out(JT, b, dJT); s.out(X, b * nx * (size_t)(T + 1), dX); s.out(U, b * nu * (size_t)T, dU); s.out(status, b, dst); s.out(iters, b, dit);
    int rc = s.upload();
    if (!rc) rc = lqmpc_controller_rollout_dev(c, T, dx0, dAt, dBt, true_per_instance, dJT, dX, dU, dst, dit);
    return rc ? rc : s.finish();
}

int lqmpc_controller_reset(lqmpc_controller *c)
{
    if (!c) return fail(LQMPC_ERR_BAD_ARG, "controller is NULL");
    if (!c->face) return 0;
    HIP_TRY(hipSetDevice(c->h->device));
    HIP_TRY(hipMemsetAsync(c->face, 0, (size_t)c->Bsz * ctl_sizes(c).face_words * sizeof(unsigned long long), c->h->stream));
    return 0;
}

int lqmpc_controller_set_reference(lqmpc_controller *c, const double *x_ref, const double *u_ref)
{
    if (!c) return fail(LQMPC_ERR_BAD_ARG, "controller is NULL");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    // the controller's own copies: every later step packs the shared block from them, and the caller's arrays are free at once
    c->has_xref = x_ref != nullptr;
    c->has_uref = u_ref != nullptr;
    if (x_ref) c->xref.assign(x_ref, x_ref + c->nx * c->N); else c->xref.clear();
    if (u_ref) c->uref.assign(u_ref, u_ref + c->nu * c->N); else c->uref.clear();
    if (!c->fast) return 0;
    // records: v_r is the one entry that depends on the references.  The shared block goes up as for a step (pinned staging, ordered
    // on the stream), then one launch rewrites v_r in place -- behind every step enqueued so far, in front of every later one.
    KParams p;
    Plan pl;
    int rc = ctl_prepare(c, ctl_call(c), p, pl);
    if (rc) return rc;
    if (!(c->wg ? lqmpc::launch_wg_ctl_retarget(p, h->stream) : lqmpc::launch_ctl_retarget(p, h->stream)))
        return fail(LQMPC_ERR_HIP, "controller retarget kernel launch failed");
    HIP_TRY(hipGetLastError());
    return 0;
}

// New models for `count` instances (the update's arrays instance-minor over count): the controller's copies of A and B, then the
// factor launch of create over the update as if it were a batch of count instances, its records redirected through didx.  Everything
// is enqueued on the handle's stream; nothing is allocated and nothing waits.
int lqmpc_controller_set_model_dev(lqmpc_controller *c, int64_t count, const int32_t *didx, const double *dA, const double *dB)
{
    if (!c) return fail(LQMPC_ERR_BAD_ARG, "controller is NULL");
    if (count == 0) return 0;
    if (count < 0 || count > c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "count must be in [0, Bsz]");
    if (!didx && count != c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "idx == NULL replaces every model: count must equal Bsz");
    if (!dA || !dB) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    const int nx = c->nx, nu = c->nu;
    // the plan and the shared block of the controller's own batch, as at create and at every step: the factor launch is sized by
    // p.Bsz alone and takes nothing from the plan, so a small update runs the kernel the whole batch was factored by.  The shared
    // block holds the references last given by set_reference: v_r of the rewritten records is computed from those.
    KParams p;
    Plan pl;
    int rc = c->fast ? ctl_prepare(c, ctl_call(c), p, pl) : 0;
    if (rc) return rc;
    if (c->A) {
        // (a workgroup-record controller keeps no copies: its records hold A and B)
        if (didx) lqmpc::launch_ctl_scatter_model((double *)c->A, (double *)c->B, dA, dB, didx, nx, nu, count, c->Bsz, h->stream);
        else {
            const size_t b = (size_t)c->Bsz;
            HIP_TRY(hipMemcpyAsync(c->A, dA, b * nx * nx * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(c->B, dB, b * nx * nu * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        }
        HIP_TRY(hipGetLastError());
    }
    if (!c->fast) return 0;
    p.A = dA; p.B = dB; p.Bsz = count;
    p.ctl_idx = didx;
    p.mode = lqmpc::MODE_CTL_FACTOR;
    return ctl_launch(c, p);
}

int lqmpc_controller_set_model(lqmpc_controller *c, int64_t count, const int32_t *idx, const double *A, const double *B)
{
    if (!c) return fail(LQMPC_ERR_BAD_ARG, "controller is NULL");
    if (count == 0) return 0;
    if (count < 0 || count > c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "count must be in [0, Bsz]");
    if (!idx && count != c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "idx == NULL replaces every model: count must equal Bsz");
    if (!A || !B) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (idx) {
        // distinct and in range, before anything is enqueued
        std::vector<char> seen((size_t)c->Bsz, 0);
        for (int64_t j = 0; j < count; ++j) {
            if (idx[j] < 0 || idx[j] >= c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "idx holds an instance outside [0, Bsz)");
            if (seen[(size_t)idx[j]]) return fail(LQMPC_ERR_BAD_ARG, "idx holds an instance twice");
            seen[(size_t)idx[j]] = 1;
        }
    }
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t m = (size_t)count, nx = (size_t)c->nx, nu = (size_t)c->nu;
    const int32_t *didx;
    const double *dA, *dB;
    s.in(idx, m, didx); s.in(A, m * nx * nx, dA); s.in(B, m * nx * nu, dB);
    int rc = s.upload();
    if (!rc) rc = lqmpc_controller_set_model_dev(c, count, didx, dA, dB);
    if (rc) return rc;
    // the staging is the handle's and the caller may overwrite A, B and idx as soon as this returns: wait, as create does
    return s.finish();
}

int64_t lqmpc_controller_bytes(const lqmpc_controller *c) { return c ? (int64_t)c->bytes : 0; }

const char *lqmpc_controller_kernel(const lqmpc_controller *c) { return c ? c->name.c_str() : "none"; }

int lqmpc_controller_destroy(lqmpc_controller *c)
{
    if (!c) return 0;
    (void)hipSetDevice(c->h->device);
    (void)hipStreamSynchronize(c->h->stream);
    if (c->h->last_owner == c->id) set_last_kernel(c->h, "none");
    ctl_free(c);
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Prepared controller for polytopic input constraints (kernels: lqmpc_poly.hip, launch_poly_ctl): one record [A | B | W | Jp] per
// instance in HBM, and the controller's own device copy of the shared block -- the one-shot calls overwrite the handle's.
struct lqmpc_poly_controller {
    lqmpc_handle *h = nullptr;
    uint64_t id = 0;                          // what the handle remembers of the controller that set last_kernel
    double eps = 0.0;                         // the handle's option when the controller was made
    int nx = 0, nu = 0, N = 0, m = 0, max_iter = 0;
    int64_t Bsz = 0;
    lqmpc::PolyOff so{};
    std::vector<double> sh_host;              // [Q | R | P | Fu | xref | uref | At | Bt]: what the device copy holds or is about to
    void *sh = nullptr, *rec = nullptr;
    void *vn = nullptr;                       // V_N of a step whose caller passed NULL (the kernel always writes it)
    long long rstride = 0;
    size_t bytes = 0;
    HostBuf pin[2];                           // pinned sources of the block's uploads, taken in turn (as the handle's shared_pin)
    int turn = 0;
};

namespace {

void pctl_free(lqmpc_poly_controller *c)
{
    for (void *q : {c->sh, c->rec, c->vn}) if (q) (void)hipFree(q);
    for (HostBuf &hb : c->pin) {
        if (hb.p) (void)hipHostFree(hb.p);
        if (hb.ev) (void)hipEventDestroy(hb.ev);
    }
    delete c;
}

int pctl_alloc(lqmpc_poly_controller *c, void **q, size_t bytes)
{
    const hipError_t e = hipMalloc(q, bytes);
    if (e != hipSuccess) { *q = nullptr; return fail(LQMPC_ERR_ALLOC, std::string("hipMalloc (polytope controller): ") + hipGetErrorString(e)); }
    c->bytes += bytes;
    return 0;
}

// doubles [off, off + count) of sh_host on their way to the device copy, ordered on the stream; no allocation after create
int pctl_upload(lqmpc_poly_controller *c, size_t off, size_t count)
{
    const size_t bytes = count * sizeof(double);
    HostBuf &hb = c->pin[c->turn ^= 1];
    const int rc = ensure_host(hb, c->sh_host.size() * sizeof(double));
    if (rc) return rc;
    if (hb.ev_valid) HIP_TRY(hipEventSynchronize(hb.ev));
    memcpy(hb.p, c->sh_host.data() + off, bytes);
    HIP_TRY(hipMemcpyAsync((double *)c->sh + off, hb.p, bytes, hipMemcpyHostToDevice, c->h->stream));
    HIP_TRY(hipEventRecord(hb.ev, c->h->stream));
    hb.ev_valid = true;
    return 0;
}

lqmpc::PolyParams pctl_params(const lqmpc_poly_controller *c)
{
    lqmpc::PolyParams p{};
    p.nx = c->nx; p.nu = c->nu; p.N = c->N; p.m = c->m; p.T = 0; p.max_iter = c->max_iter; p.eps = c->eps; p.Bsz = c->Bsz;
    p.sh = (const double *)c->sh; p.so = c->so;
    p.rec = (double *)c->rec; p.rstride = c->rstride; p.nrec = c->Bsz; p.idx = nullptr;
    return p;
}

int pctl_launch(lqmpc_poly_controller *c, const lqmpc::PolyParams &p, int what)
{
    const char *name = nullptr;
    if (!lqmpc::launch_poly_ctl(p, what, c->h->stream, &name)) return fail(LQMPC_ERR_HIP, "the polytope controller kernel's launch failed");
    HIP_TRY(hipGetLastError());
    set_last_kernel(c->h, name, c->id);
    return 0;
}

// the factor launch over an update of `count` models (device, instance-minor over count), its records redirected through didx
int pctl_factor(lqmpc_poly_controller *c, int64_t count, const int32_t *didx, const double *dA, const double *dB)
{
    lqmpc::PolyParams p = pctl_params(c);
    p.Bsz = count; p.A = dA; p.B = dB; p.idx = didx;
    return pctl_launch(c, p, lqmpc::POLY_CTL_FACTOR);
}

int pctl_create(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B, bool on_device, const double *Q,
                const double *R, const double *P, const double *Fu, int m, const double *x_ref, const double *u_ref, int max_iter,
                lqmpc_poly_controller **out)
{
    if (out) *out = nullptr;
    int rc = poly_check(h, nx, nu, N, Bsz, 0, false, A, B, Q, R, P, Fu, m, A, nullptr, nullptr, max_iter, out, out);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    lqmpc_poly_controller *c = new lqmpc_poly_controller();
    c->h = h; c->id = ++h->ctl_ids; c->eps = h->opt.eps; c->nx = nx; c->nu = nu; c->N = N; c->m = m; c->max_iter = max_iter; c->Bsz = Bsz;
    c->rstride = lqmpc::poly_rec_layout(nx, nu, N).stride;
    std::vector<double> &sh = c->sh_host;
    auto put = [&](const double *src, int count) {
        int off = (int)sh.size();
        sh.resize(sh.size() + count, 0.0);
        if (src) memcpy(sh.data() + off, src, sizeof(double) * count);
        return off;
    };
    c->so.Q = put(Q, nx * nx);
    c->so.R = put(R, nu * nu);
    c->so.P = put(P, nx * nx);
    c->so.Fu = put(Fu, m * nu);
    c->so.xref = put(x_ref, nx * N);
    c->so.uref = put(u_ref, nu * N);
    c->so.At = put(nullptr, nx * nx);
    c->so.Bt = put(nullptr, nx * nu);
    const size_t rec_bytes = (size_t)Bsz * (size_t)c->rstride * sizeof(double);
    rc = pctl_alloc(c, &c->sh, sh.size() * sizeof(double));
    if (!rc) rc = pctl_alloc(c, &c->rec, rec_bytes);
    if (!rc) rc = pctl_alloc(c, &c->vn, (size_t)Bsz * sizeof(double));
    for (HostBuf &hb : c->pin) if (!rc) rc = ensure_host(hb, sh.size() * sizeof(double));
    if (!rc) rc = pctl_upload(c, 0, sh.size());
    if (rc) { pctl_free(c); return rc; }
    // (the padding behind a record is never read; zeroed so that the controller's memory is defined everywhere)
    hipError_t e = hipMemsetAsync(c->rec, 0, rec_bytes, h->stream);
    if (e != hipSuccess) { pctl_free(c); return fail(LQMPC_ERR_HIP, std::string("polytope controller set-up: ") + hipGetErrorString(e)); }
    if (on_device) rc = pctl_factor(c, Bsz, nullptr, A, B);
    else {
        Stager s{h};
        const double *dA, *dB;
        s.in(A, (size_t)Bsz * nx * nx, dA); s.in(B, (size_t)Bsz * nx * nu, dB);
        rc = s.upload();
        if (!rc) rc = pctl_factor(c, Bsz, nullptr, dA, dB);
    }
    // the caller may overwrite A and B as soon as this returns
    if (!rc) {
        e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(LQMPC_ERR_HIP, std::string("polytope controller set-up: ") + hipGetErrorString(e));
    }
    if (rc) { pctl_free(c); return rc; }
    *out = c;
    return 0;
}

}  // namespace

extern "C" {

int64_t lqmpc_poly_controller_record_bytes(int nx, int nu, int N)
{
    const int rc = check_dims(nx, nu, N, 1);
    if (rc) return rc;
    if (N * nu > POLY_MAX_NVAR) return fail(LQMPC_ERR_UNSUPPORTED, "the polytope kernels serve N*nu<=64");
    return (int64_t)sizeof(double) * lqmpc::poly_rec_layout(nx, nu, N).stride;
}

int lqmpc_poly_controller_create(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *A, const double *B, const double *Q,
                                 const double *R, const double *P, const double *Fu, int m, const double *x_ref, const double *u_ref,
                                 int max_iter, lqmpc_poly_controller **out)
{
    return pctl_create(h, nx, nu, N, Bsz, A, B, false, Q, R, P, Fu, m, x_ref, u_ref, max_iter, out);
}

int lqmpc_poly_controller_create_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, const double *dA, const double *dB,
                                     const double *Q, const double *R, const double *P, const double *Fu, int m, const double *x_ref,
                                     const double *u_ref, int max_iter, lqmpc_poly_controller **out)
{
    return pctl_create(h, nx, nu, N, Bsz, dA, dB, true, Q, R, P, Fu, m, x_ref, u_ref, max_iter, out);
}

int lqmpc_poly_controller_step_dev(lqmpc_poly_controller *c, const double *dx, double *du0, double *dVN, double *dUplan, double *dXplan,
                                   double *dlam, int32_t *dstatus, int32_t *diters)
{
    if (!c || !dx || !du0) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->h->device));
    lqmpc::PolyParams p = pctl_params(c);
    p.x0 = dx;
    p.u0 = du0; p.VN = dVN ? dVN : (double *)c->vn; p.Uplan = dUplan; p.Xplan = dXplan; p.lam = dlam; p.status = dstatus; p.iters = diters;
    return pctl_launch(c, p, lqmpc::POLY_CTL_STEP);
}

int lqmpc_poly_controller_step(lqmpc_poly_controller *c, const double *x, double *u0, double *VN, double *Uplan, double *Xplan, double *lam,
                               int32_t *status, int32_t *iters)
{
    if (!c || !x || !u0) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)c->Bsz, nx = (size_t)c->nx, nu = (size_t)c->nu, N = (size_t)c->N;
    const double *dx;
    double *du0, *dVN, *dUp, *dXp, *dlam;
    int32_t *dst, *dit;
    s.in(x, b * nx, dx);
    s.out(u0, b * nu, du0); s.out(VN, b, dVN); s.out(Uplan, b * nu * N, dUp); s.out(Xplan, b * nx * (N + 1), dXp);
    s.out(lam, b * (size_t)c->m * N, dlam); s.out(status, b, dst); s.out(iters, b, dit);
    int rc = s.upload();
    if (!rc) rc = lqmpc_poly_controller_step_dev(c, dx, du0, dVN, dUp, dXp, dlam, dst, dit);
    return rc ? rc : s.finish();
}

// T closed-loop steps of every instance from the records, in one launch; read-only on the records.  A shared plant is a host pointer
// in both flavours: staged in the controller's own shared block.
int lqmpc_poly_controller_rollout_dev(lqmpc_poly_controller *c, int T, const double *dx0, const double *A_true, const double *B_true,
                                      int true_per_instance, double *dJT, double *dX, double *dU, int32_t *dstatus, int32_t *diters)
{
    if (!c || !dx0 || !A_true || !B_true || !dJT) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    HIP_TRY(hipSetDevice(c->h->device));
    lqmpc::PolyParams p = pctl_params(c);
    p.T = T; p.x0 = dx0;
    p.JT = dJT; p.X = dX; p.U = dU; p.status = dstatus; p.iters = diters;
    if (true_per_instance) { p.At = A_true; p.Bt = B_true; p.sE = c->Bsz; p.sI = 1; }
    else {
        const int nx = c->nx, nu = c->nu;
        memcpy(c->sh_host.data() + c->so.At, A_true, sizeof(double) * nx * nx);
        memcpy(c->sh_host.data() + c->so.Bt, B_true, sizeof(double) * nx * nu);
        const int rc = pctl_upload(c, (size_t)c->so.At, (size_t)(nx * nx + nx * nu));      // (At and Bt are neighbours in the block)
        if (rc) return rc;
        p.At = p.sh + c->so.At; p.Bt = p.sh + c->so.Bt; p.sE = 1; p.sI = 0;
    }
    return pctl_launch(c, p, lqmpc::POLY_CTL_ROLLOUT);
}

int lqmpc_poly_controller_rollout(lqmpc_poly_controller *c, int T, const double *x0, const double *A_true, const double *B_true,
                                  int true_per_instance, double *JT, double *X, double *U, int32_t *status, int32_t *iters)
{
    if (!c || !x0 || !A_true || !B_true || !JT) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (T < 1 || T > 100000) return fail(LQMPC_ERR_BAD_ARG, "T must be in [1,100000]");
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t b = (size_t)c->Bsz, nx = (size_t)c->nx, nu = (size_t)c->nu;
    const double *dx0, *dAt = A_true, *dBt = B_true;
    double *dJT, *dX, *dU;
    int32_t *dst, *dit;
    s.in(x0, b * nx, dx0);
    if (true_per_instance) { s.in(A_true, b * nx * nx, dAt); s.in(B_true, b * nx * nu, dBt); }
    s.out(JT, b, dJT); s.out(X, b * nx * (size_t)(T + 1), dX); s.out(U, b * nu * (size_t)T, dU); s.out(status, b, dst); s.out(iters, b, dit);
    int rc = s.upload();
    if (!rc) rc = lqmpc_poly_controller_rollout_dev(c, T, dx0, dAt, dBt, true_per_instance, dJT, dX, dU, dst, dit);
    return rc ? rc : s.finish();
}

// No part of a record depends on the references: the two reference blocks of the controller's shared copy are rewritten, behind
// every step enqueued so far and in front of every later one.  No kernel.
int lqmpc_poly_controller_set_reference(lqmpc_poly_controller *c, const double *x_ref, const double *u_ref)
{
    if (!c) return fail(LQMPC_ERR_BAD_ARG, "controller is NULL");
    HIP_TRY(hipSetDevice(c->h->device));
    const size_t nxr = (size_t)c->nx * c->N, nur = (size_t)c->nu * c->N;
    double *xr = c->sh_host.data() + c->so.xref, *ur = c->sh_host.data() + c->so.uref;
    if (x_ref) memcpy(xr, x_ref, sizeof(double) * nxr); else std::fill(xr, xr + nxr, 0.0);
    if (u_ref) memcpy(ur, u_ref, sizeof(double) * nur); else std::fill(ur, ur + nur, 0.0);
    return pctl_upload(c, (size_t)c->so.xref, nxr + nur);                                   // (xref and uref are neighbours in the block)
}

// New models for `count` instances: the factor launch of create over the update, its records redirected through didx.  The records
// hold the controller's copies of A and B, so the launch refreshes those too; a record that is not listed is not touched.
int lqmpc_poly_controller_set_model_dev(lqmpc_poly_controller *c, int64_t count, const int32_t *didx, const double *dA, const double *dB)
{
    if (!c) return fail(LQMPC_ERR_BAD_ARG, "controller is NULL");
    if (count == 0) return 0;
    if (!dA || !dB) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (count < 0 || count > c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "count must be in [0, Bsz]");
    if (!didx && count != c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "idx == NULL replaces every model: count must equal Bsz");
    HIP_TRY(hipSetDevice(c->h->device));
    return pctl_factor(c, count, didx, dA, dB);
}

int lqmpc_poly_controller_set_model(lqmpc_poly_controller *c, int64_t count, const int32_t *idx, const double *A, const double *B)
{
    if (!c) return fail(LQMPC_ERR_BAD_ARG, "controller is NULL");
    if (count == 0) return 0;
    if (!A || !B) return fail(LQMPC_ERR_BAD_ARG, "NULL argument");
    if (count < 0 || count > c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "count must be in [0, Bsz]");
    if (!idx && count != c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "idx == NULL replaces every model: count must equal Bsz");
    if (idx) {
        // distinct and in range, before anything is enqueued
        std::vector<char> seen((size_t)c->Bsz, 0);
        for (int64_t j = 0; j < count; ++j) {
            if (idx[j] < 0 || idx[j] >= c->Bsz) return fail(LQMPC_ERR_BAD_ARG, "idx holds an instance outside [0, Bsz)");
            if (seen[(size_t)idx[j]]) return fail(LQMPC_ERR_BAD_ARG, "idx holds an instance twice");
            seen[(size_t)idx[j]] = 1;
        }
    }
    lqmpc_handle *h = c->h;
    HIP_TRY(hipSetDevice(h->device));
    Stager s{h};
    const size_t k = (size_t)count, nx = (size_t)c->nx, nu = (size_t)c->nu;
    const int32_t *didx;
    const double *dA, *dB;
    s.in(idx, k, didx); s.in(A, k * nx * nx, dA); s.in(B, k * nx * nu, dB);
    int rc = s.upload();
    if (!rc) rc = lqmpc_poly_controller_set_model_dev(c, count, didx, dA, dB);
    if (rc) return rc;
    // the staging is the handle's and the caller may overwrite A, B and idx as soon as this returns: wait, as create does
    return s.finish();
}

int64_t lqmpc_poly_controller_bytes(const lqmpc_poly_controller *c) { return c ? (int64_t)c->bytes : 0; }

const char *lqmpc_poly_controller_kernel(const lqmpc_poly_controller *c) { return c ? "lqmpc_poly_ctl_step_kernel" : "none"; }

int lqmpc_poly_controller_destroy(lqmpc_poly_controller *c)
{
    if (!c) return 0;
    (void)hipSetDevice(c->h->device);
    (void)hipStreamSynchronize(c->h->stream);
    if (c->h->last_owner == c->id) set_last_kernel(c->h, "none");
    pctl_free(c);
    return 0;
}

}  // extern "C"
