// lqmpc_probe.h -- the difficulty probe of the ordered rollouts (options.order): one launch computes a key per instance, reserves
// its position inside its difficulty bucket and, under the free-response key, stages the instance-major [A | B | x0] records the
// sorted walk reads.
// Device code only (no standard-library header): included by lqmpc_spec.hip for the prebuilt shapes and compiled at run time for the
// others (lqmpc_jit.hip).
#pragma once
#include "lqmpc_common.h"

namespace lqmpc {

// ---------------- difficulty probe (options.order) ----------------
// One instance per lane, PROBE_WG instances per workgroup.  Two keys: for rollouts on a shared plant a clipped roll of that plant
// (order_roll, below); otherwise the largest stage gradient of the FREE response over the horizon, in
// units of what one input can counter:  max_r max_k |B_k' Q A^(r+1) x0| / ((B'QB + R)_kk h_k).
// It needs neither condensing nor a factorisation (240 FMAs per instance at C3) and orders the batch
// almost as well as the exact overshoot of the unconstrained minimiser (20.5 % vs 19.8 % of wave-steps
// left with a constrained instance on C3; natural order 48.7 %).  A heuristic: it only decides which
// instances share a wavefront, never a result.
//
// Where the host asks for them (p.stage set: build_order) the same pass stages the instance-major [A | B | x0] records the sorted
// walk reads.  Under the free-response key it has A and B in registers anyway.  The roll key reads nothing of an instance but x0, so
// with p.stage null under it the launch is the key's chain of dependent latencies alone -- the x0 load, the roll, one LDS and one
// global round of atomics, the store: no A, no B -- and the sorted walk reads the instance-minor arrays through its permutation
// (what that saves, and what staging from workgroups of their own in the same launch measured: DESIGN.md section 4.3b).
//
// The records of a workgroup's instances are one contiguous piece of p.stage.  Where it fits in LDS (PROBE_WG records: C3's 56 KB)
// the workgroup lays the piece out there and copies it out 16 bytes a lane, whole 64-byte lines a wavefront -- a lane storing its own
// record field by field touches 64 lines with every store instruction (1.8 M eight-byte requests at C3 x 65 536).  Larger records
// are stored by their lanes as before.
//
// Positions inside a bucket: the workgroup counts its instances per bucket in LDS (the LDS atomic hands every lane its rank), then
// reserves each non-empty bucket's run with ONE global atomic, all of them in flight at once.
template <int NX, int NU>
struct ProbeRec {
    static constexpr int REC = NX * NX + NX * NU + NX;
    static constexpr bool DENSE = PROBE_WG * REC * 8 <= 56 * 1024;      // (+ 2 KB of counters: inside the 64 KB of a static allocation)
};

// The probe of the wide states (9 <= NX <= 16, run-time compiled only): the same keys and the same bookkeeping as probe_body below, but
// nothing that is NX x NX is held in registers -- 16 x 16 doubles are a lane's whole register file.  Records are copied element by
// element (they never fit the LDS piece); the roll key reads plant and gain -- scalar loads of the shared block -- where the step uses
// them (`zs`: an opaque zero set in every step, so that the loads stay inside the loop); the free-response key reads A four rows at a
// time (`bz`: an opaque copy of the instance index, so that the 256 addresses are formed in the loop and not held across it).
template <int NX, int NU, int N>
__device__ __forceinline__ void probe_body_wide(const KParams &p)
{
    constexpr int REC = ProbeRec<NX, NU>::REC;
    static_assert(NX > 8 && !ProbeRec<NX, NU>::DENSE, "wide records do not fit the LDS piece");
    __shared__ int cnt[ORDER_BUCKETS];
    const long long Bsz = p.Bsz;
    const int tid = threadIdx.x;
    const long long b0 = (long long)blockIdx.x * PROBE_WG, bt = b0 + tid;
    const bool live = bt < Bsz;
    const long long b = live ? bt : Bsz - 1;            // surplus lanes of the last workgroup shadow the last instance and write nothing
    if (p.hist_next) {
        const long long total = (long long)gridDim.x * PROBE_WG;
        for (long long e = bt; e < (long long)ORDER_BUCKETS * ORDER_PAD; e += total) p.hist_next[e] = 0;
    }
    if (p.fail_count && bt == 0) { p.fail_count[0] = 0; p.fail_count[1] = 0; }
#pragma unroll
    for (int k = 0; k < ORDER_BUCKETS / PROBE_WG; ++k) cnt[tid + k * PROBE_WG] = 0;
    const double *sh = p.sh;
    double x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = p.x0[(long long)i * Bsz + b];
    if (p.stage && live) {
#pragma unroll 1
        for (int e = 0; e < NX * NX; ++e) p.stage[b * REC + e] = p.A[(long long)e * Bsz + b];
#pragma unroll 1
        for (int e = 0; e < NX * NU; ++e) p.stage[b * REC + NX * NX + e] = p.B[(long long)e * Bsz + b];
#pragma unroll
        for (int i = 0; i < NX; ++i) p.stage[b * REC + NX * NX + NX * NU + i] = x[i];
    }
    __syncthreads();                                    // the counters are zero
    int raw;
    if (p.order_roll) {
        double hk[NU], nhk[NU], hinv[NU];
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            hk[k] = 0.5 * (sh[p.so.ub + k] - sh[p.so.lb + k]);
            nhk[k] = -hk[k];
            hinv[k] = 1.0 / hk[k];
        }
        const int Ts = p.T < 31 ? p.T : 31;              // (16 (Ts) + 15 < ORDER_BUCKETS)
        int last = 0, zs = 0;
        double marg = 0.0;
#pragma unroll 1
        for (int t = 0; t < Ts; ++t) {
            asm volatile("" : "+s"(zs));
            double u[NU], m = 0.0;
#pragma unroll
            for (int k = 0; k < NU; ++k) {
                double uk = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) uk = __builtin_fma(-sh[p.so.Kg + k * NX + j + zs], x[j], uk);
                m = fmax(m, fabs(uk) * hinv[k]);
                u[k] = fmin(fmax(uk, nhk[k]), hk[k]);
            }
            const bool over = m > 1.0;
            last = over ? t + 1 : last;
            marg = (over || t == 0) ? m : marg;
            double xn[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) acc = __builtin_fma(sh[p.so.At + i * NX + j + zs], x[j], acc);
#pragma unroll
                for (int k = 0; k < NU; ++k) acc = __builtin_fma(sh[p.so.Bt + i * NU + k + zs], u[k], acc);
                xn[i] = acc;
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = xn[i];
            if (__ballot(t - last < 3) == 0ull) break;   // no lane of the wavefront saturated in the last three steps: they have settled
        }
        double xs = 0.0;                                 // (a NaN anywhere has reached every component by now: first in the order)
#pragma unroll
        for (int i = 0; i < NX; ++i) xs += fabs(x[i]);
        const double g = last > 0 ? 1.0 - 1.0 / marg : fmin(marg, 0.999);
        raw = (xs < 1e300 && marg == marg) ? 16 * last + (int)(16.0 * g) : ORDER_BUCKETS - 1;
    } else {
        double QB[NX][NU], dinv[NU];        // Q B and 1 / ((B'QB + R)_kk h_k)
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int k = 0; k < NU; ++k) {
                double t = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) t = __builtin_fma(sh[p.so.Q + i * NX + j], p.B[(long long)(j * NU + k) * Bsz + b], t);
                QB[i][k] = t;
            }
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            double t = sh[p.so.R + k * NU + k];
#pragma unroll
            for (int i = 0; i < NX; ++i) t = __builtin_fma(p.B[(long long)(i * NU + k) * Bsz + b], QB[i][k], t);
            dinv[k] = 1.0 / (t * 0.5 * (sh[p.so.ub + k] - sh[p.so.lb + k]));
        }
        double key = 0.0;
#pragma unroll 1
        for (int r = 0; r < N; ++r) {
            long long bz = b;
            asm volatile("" : "+v"(bz));
            double xn[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                if (i % 4 == 0) asm volatile("" ::: "memory");      // (four rows of loads in flight, not the whole matrix)
                double t = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) t = __builtin_fma(p.A[(long long)(i * NX + j) * Bsz + bz], x[j], t);
                xn[i] = t;
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = xn[i];
#pragma unroll
            for (int k = 0; k < NU; ++k) {
                double g = 0.0;
#pragma unroll
                for (int i = 0; i < NX; ++i) g = __builtin_fma(QB[i][k], x[i], g);
                key = fmax(key, fabs(g) * dinv[k]);
            }
        }
        const double kk = (key == key) ? key : 1e300;
        raw = (int)((unsigned)__double2hiint(kk) >> 16) - ((1023 - 2) << 4);      // (the buckets of probe_body)
    }
    const int bucket = raw < 0 ? 0 : (raw > ORDER_BUCKETS - 1 ? ORDER_BUCKETS - 1 : raw);
    const int rank = live ? atomicAdd(&cnt[bucket], 1) : 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ORDER_BUCKETS / PROBE_WG; ++k) {
        const int e = tid + k * PROBE_WG;
        const int c = cnt[e];
        if (c) cnt[e] = atomicAdd(&p.hist[e * ORDER_PAD], c);
    }
    __syncthreads();
    if (live) ((int2 *)p.key)[b] = make_int2(bucket, cnt[bucket] + rank);
}

template <int NX, int NU, int N>
__device__ __forceinline__ void probe_body(const KParams &p)
{
    constexpr int REC = ProbeRec<NX, NU>::REC;
    constexpr bool DENSE = ProbeRec<NX, NU>::DENSE;
    __shared__ int cnt[ORDER_BUCKETS];          // instances of this workgroup per bucket, then the start of their run in the bucket
    __shared__ __attribute__((aligned(16))) double tr[DENSE ? PROBE_WG * REC : 2];
    const long long Bsz = p.Bsz;
    const int tid = threadIdx.x;
    const long long b0 = (long long)blockIdx.x * PROBE_WG, bt = b0 + tid;
    const bool live = bt < Bsz;
    const long long b = live ? bt : Bsz - 1;            // surplus lanes of the last workgroup shadow the last instance and write nothing
    // housekeeping that used to be a fill launch per call: the counters the NEXT call's probe will count into (the two sets
    // alternate; the last reader of that set, the previous call's scatter, is long done) and this call's hand-back count
    if (p.hist_next) {
        const long long total = (long long)gridDim.x * PROBE_WG;
        for (long long e = bt; e < (long long)ORDER_BUCKETS * ORDER_PAD; e += total) p.hist_next[e] = 0;
    }
    if (p.fail_count && bt == 0) { p.fail_count[0] = 0; p.fail_count[1] = 0; }
#pragma unroll
    for (int k = 0; k < ORDER_BUCKETS / PROBE_WG; ++k) cnt[tid + k * PROBE_WG] = 0;
    const double *sh = p.sh;
    double A[NX][NX] = {}, Bm[NX][NU] = {}, x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = p.x0[(long long)i * Bsz + b];
    if (!p.order_roll || p.stage) {                     // (uniform) the roll key needs x0 only: A and B only to stage them
#pragma unroll
        for (int i = 0; i < NX; ++i) {
#pragma unroll
            for (int j = 0; j < NX; ++j) A[i][j] = p.A[(long long)(i * NX + j) * Bsz + b];
#pragma unroll
            for (int k = 0; k < NU; ++k) Bm[i][k] = p.B[(long long)(i * NU + k) * Bsz + b];
        }
    }
    if constexpr (DENSE) {
        if (p.stage) {
#pragma unroll
            for (int i = 0; i < NX; ++i) {
#pragma unroll
                for (int j = 0; j < NX; ++j) tr[tid * REC + i * NX + j] = A[i][j];
#pragma unroll
                for (int k = 0; k < NU; ++k) tr[tid * REC + NX * NX + i * NU + k] = Bm[i][k];
                tr[tid * REC + NX * NX + NX * NU + i] = x[i];
            }
        }
    } else if (p.stage && live) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
#pragma unroll
            for (int j = 0; j < NX; ++j) p.stage[b * REC + i * NX + j] = A[i][j];
#pragma unroll
            for (int k = 0; k < NU; ++k) p.stage[b * REC + NX * NX + i * NU + k] = Bm[i][k];
            p.stage[b * REC + NX * NX + NX * NU + i] = x[i];
        }
    }
    __syncthreads();                                    // the counters are zero, the records lie in LDS
    if constexpr (DENSE) {
        if (p.stage) {
            // the workgroup's piece: nrec records from b0 on, 16-byte aligned (PROBE_WG * REC doubles a workgroup), copied in pairs
            const long long left = Bsz - b0;
            const int nd = (int)(left < PROBE_WG ? left : PROBE_WG) * REC;
            double *dst = p.stage + b0 * REC;
#pragma unroll
            for (int k = 0; k < (REC + 1) / 2; ++k) {
                const int e = 2 * (tid + k * PROBE_WG);
                if (e + 1 < nd) *(double2 *)(dst + e) = *(const double2 *)(tr + e);
                else if (e < nd) dst[e] = tr[e];
            }
        }
    }
    int raw;
    if (p.order_roll) {
        // Rollouts on a shared plant (zero references, centred box): the instance's own closed loop, approximately -- the PLANT rolled
        // forward from x0 under the first gain of the N-stage problem on it (host: so.Kg), inputs clipped.  Key = the last step whose
        // input saturates (the MPC steps up to there are the constrained ones), 16ths of a margin behind it: 1 - 1/m at that step,
        // or m at x0 where no step saturates (m = max_k |u_k| / h_k).  Wave-steps with a constrained instance at C3, four instances
        // per wavefront in this order: 15.1 % (the free-response key below: 18.3 %, the true count of constrained steps: 14.8 %,
        // natural order: 29.3 %; hard mix 67.3 / 78.6 / 66.2 / 91.5 %: tests/dev/order_keys.py).  ~1000 FMAs per instance on
        // scalar operands.
        double At[NX][NX], Bt[NX][NU], Kg[NU][NX], hk[NU], nhk[NU], hinv[NU];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
#pragma unroll
            for (int j = 0; j < NX; ++j) At[i][j] = sh[p.so.At + i * NX + j];
#pragma unroll
            for (int k = 0; k < NU; ++k) Bt[i][k] = sh[p.so.Bt + i * NU + k];
        }
#pragma unroll
        for (int k = 0; k < NU; ++k) {
#pragma unroll
            for (int j = 0; j < NX; ++j) Kg[k][j] = sh[p.so.Kg + k * NX + j];
            hk[k] = 0.5 * (sh[p.so.ub + k] - sh[p.so.lb + k]);
            nhk[k] = -hk[k];
            hinv[k] = 1.0 / hk[k];
        }
        const int Ts = p.T < 31 ? p.T : 31;              // (16 (Ts) + 15 < ORDER_BUCKETS)
        int last = 0;
        double marg = 0.0;
#pragma unroll 1
        for (int t = 0; t < Ts; ++t) {
            double u[NU], m = 0.0;
#pragma unroll
            for (int k = 0; k < NU; ++k) {
                double uk = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) uk = __builtin_fma(-Kg[k][j], x[j], uk);
                m = fmax(m, fabs(uk) * hinv[k]);
                u[k] = fmin(fmax(uk, nhk[k]), hk[k]);
            }
            const bool over = m > 1.0;
            last = over ? t + 1 : last;
            marg = (over || t == 0) ? m : marg;
            double xn[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) acc = __builtin_fma(At[i][j], x[j], acc);
#pragma unroll
                for (int k = 0; k < NU; ++k) acc = __builtin_fma(Bt[i][k], u[k], acc);
                xn[i] = acc;
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = xn[i];
            if (__ballot(t - last < 3) == 0ull) break;   // no lane of the wavefront saturated in the last three steps: they have settled
        }
        double xs = 0.0;                                 // (a NaN anywhere has reached every component by now: first in the order)
#pragma unroll
        for (int i = 0; i < NX; ++i) xs += fabs(x[i]);
        const double g = last > 0 ? 1.0 - 1.0 / marg : fmin(marg, 0.999);
        raw = (xs < 1e300 && marg == marg) ? 16 * last + (int)(16.0 * g) : ORDER_BUCKETS - 1;
    } else {
        double QB[NX][NU], dinv[NU];        // Q B and 1 / ((B'QB + R)_kk h_k)
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int k = 0; k < NU; ++k) {
                double t = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) t = __builtin_fma(sh[p.so.Q + i * NX + j], Bm[j][k], t);
                QB[i][k] = t;
            }
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            double t = sh[p.so.R + k * NU + k];
#pragma unroll
            for (int i = 0; i < NX; ++i) t = __builtin_fma(Bm[i][k], QB[i][k], t);
            dinv[k] = 1.0 / (t * 0.5 * (sh[p.so.ub + k] - sh[p.so.lb + k]));
        }
        double key = 0.0;
#pragma unroll 1
        for (int r = 0; r < N; ++r) {
            double xn[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                double t = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) t = __builtin_fma(A[i][j], x[j], t);
                xn[i] = t;
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = xn[i];
#pragma unroll
            for (int k = 0; k < NU; ++k) {
                double g = 0.0;
#pragma unroll
                for (int i = 0; i < NX; ++i) g = __builtin_fma(QB[i][k], x[i], g);
                key = fmax(key, fabs(g) * dinv[k]);
            }
        }
        const double kk = (key == key) ? key : 1e300;
        // The order only has to group similar instances, hardest first: a bucket sort on the logarithm of the key (exponent and
        // four mantissa bits of the fp64: 16 buckets per binade, clamped to [2^-2, 2^30): an instance whose key is below 1/4 never meets its bounds; finer buckets cost more atomics
        // than they save in the rollout.  lqmpc_order_scatter_kernel turns (bucket, position) into the slot of the instance.
        raw = (int)((unsigned)__double2hiint(kk) >> 16) - ((1023 - 2) << 4);
    }
    const int bucket = raw < 0 ? 0 : (raw > ORDER_BUCKETS - 1 ? ORDER_BUCKETS - 1 : raw);
    const int rank = live ? atomicAdd(&cnt[bucket], 1) : 0;          // (LDS) my position among the workgroup's instances of my bucket
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ORDER_BUCKETS / PROBE_WG; ++k) {
        const int e = tid + k * PROBE_WG;
        const int c = cnt[e];
        if (c) cnt[e] = atomicAdd(&p.hist[e * ORDER_PAD], c);           // all the workgroup's reservations in flight at once
    }
    __syncthreads();
    if (live) ((int2 *)p.key)[b] = make_int2(bucket, cnt[bucket] + rank);
}

template <int NX, int NU, int N>
__global__ void __launch_bounds__(PROBE_WG) lqmpc_probe_kernel(KParams p) { probe_body<NX, NU, N>(p); }

}  // namespace lqmpc
