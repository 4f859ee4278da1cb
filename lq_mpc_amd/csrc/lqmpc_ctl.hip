// lqmpc_ctl.hip -- the kernels of a prepared controller (lqmpc_controller_*, include/lqmpc.h) in the 16-lane-row layout.
//
// A one-shot solve spends about half of its launch on what does not depend on the state: the backward Riccati sweep, W = P^-1, the
// gain G of the unconstrained minimiser and P.  A controller runs that once (MODE_CTL_FACTOR: the set-up of lqmpc_r16_body.h as it
// stands, then one record per instance written to HBM instead of a QP) and every step after it (MODE_CTL_STEP) starts from the record:
//   [A | B | G | v_r]   read by every step: v = G x + v_r, the test against the box, the model for V_N
//   [W]                 packed lower triangle, brought into LDS only by the instances of a wavefront that have to iterate
//   [P]                 packed lower triangle, only when an iteration takes the primal side (|A| > n / 2)
// Records are instance-major and padded to 256 bytes, so the lanes of an instance read consecutive addresses.  The iterations are the
// qp() of lqmpc_r16_body.h, not a copy; the face a step ends on is kept per instance (two 64-bit masks, with the state it was found at
// and the state the model expected next) and warm-starts the next one: shifted by one stage as the rollout shifts it when the state
// advanced, unshifted when it stayed.  MODE_CTL_ROLL runs T closed-loop steps per instance from the same record (the rollout's loop
// without its set-up; W stays in LDS once an instance has brought it in) and leaves the stored faces alone.
#include "lqmpc_r16_body.h"
#include "lqmpc_launch.h"

namespace lqmpc {

// register / LDS budget: as the one-shot kernels of the same shape (R16Build)
template <int NX, int NU, int N, int MODE, int LPI>
__global__ void __launch_bounds__(64, (R16Build<NX, NU, N, LPI>::WAVES)) lqmpc_ctl_kernel(KParams p)
{
    using C = R16<NX, NU, N, LPI, (R16Build<NX, NU, N, LPI>::OCC == 2)>;
    __shared__ double lds_raw[C::IPW * C::INST];
    r16_body<NX, NU, N, MODE, LPI, R16Build<NX, NU, N, LPI>::OCC>(p, lds_raw, (long long)blockIdx.x * C::IPW, p.Bsz);
}

// MODE_CTL_STEP with the whole plan written out (p.Uplan): a kernel of its own, so that the plain step's kernel holds none of it
template <int NX, int NU, int N, int LPI>
__global__ void __launch_bounds__(64, (R16Build<NX, NU, N, LPI>::WAVES)) lqmpc_ctl_plan_kernel(KParams p)
{
    using C = R16<NX, NU, N, LPI, (R16Build<NX, NU, N, LPI>::OCC == 2)>;
    __shared__ double lds_raw[C::IPW * C::INST];
    r16_body<NX, NU, N, MODE_CTL_STEP, LPI, R16Build<NX, NU, N, LPI>::OCC, false, true>(p, lds_raw, (long long)blockIdx.x * C::IPW, p.Bsz);
}

template <int NX, int NU, int N, int LPI>
static void launch_ctl_one(const KParams &p, hipStream_t stream)
{
    constexpr int IPW = 64 / LPI;
    const dim3 grid((unsigned)((p.Bsz + IPW - 1) / IPW));
    if (p.mode == MODE_CTL_STEP && p.Uplan) hipLaunchKernelGGL((lqmpc_ctl_plan_kernel<NX, NU, N, LPI>), grid, dim3(64), 0, stream, p);
    else if (p.mode == MODE_CTL_FACTOR) hipLaunchKernelGGL((lqmpc_ctl_kernel<NX, NU, N, MODE_CTL_FACTOR, LPI>), grid, dim3(64), 0, stream, p);
    else if (p.mode == MODE_CTL_ROLL) hipLaunchKernelGGL((lqmpc_ctl_kernel<NX, NU, N, MODE_CTL_ROLL, LPI>), grid, dim3(64), 0, stream, p);
    else hipLaunchKernelGGL((lqmpc_ctl_kernel<NX, NU, N, MODE_CTL_STEP, LPI>), grid, dim3(64), 0, stream, p);
}

// the prebuilt shapes; every other shape of the 16-lane-row domain is compiled at run time (lqmpc_jit.hip)
static const ShapeEntry g_ctl[] = {
    {4, 2, 10, 16, "lqmpc_ctl_r16_kernel<4,2,10>", launch_ctl_one<4, 2, 10, 16>},
    {2, 1, 10, 16, "lqmpc_ctl_r16_kernel<2,1,10>", launch_ctl_one<2, 1, 10, 16>},
    {4, 2, 20, 64, "lqmpc_ctl_r64_kernel<4,2,20>", launch_ctl_one<4, 2, 20, 64>},
};

static const ShapeEntry *find_ctl(int nx, int nu, int N)
{
    for (const ShapeEntry &e : g_ctl)
        if (e.nx == nx && e.nu == nu && e.N == N) return &e;
    return nullptr;
}

bool ctl_available(int nx, int nu, int N) { return find_ctl(nx, nu, N) != nullptr; }

// p.mode: MODE_CTL_FACTOR, MODE_CTL_STEP or MODE_CTL_ROLL
bool launch_ctl(const KParams &p, hipStream_t stream, const char **name)
{
    const ShapeEntry *e = find_ctl(p.nx, p.nu, p.N);
    if (!e || (p.mode != MODE_CTL_FACTOR && p.mode != MODE_CTL_STEP && p.mode != MODE_CTL_ROLL)) return false;
    e->launch(p, stream);
    if (name) *name = e->name;
    return true;
}

}  // namespace lqmpc
