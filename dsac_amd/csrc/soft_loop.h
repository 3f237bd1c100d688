// soft_loop.h -- the re-weighted refinement loop of dsac_refine_soft (k_refine.hip) and dsac_refine_rgbd (k_rgbd.hip), once: statuses, state and scratch
// layout, frame selection, the ordered chunk sum, the decision, the result write, the one-wave step kernel and the host loop of the split form.  A path is a
// POLICY type:
//   NACC, S_AT          sums per pass, and which of them is the soft count S
//   struct Src          kernel argument of the step: what the per-problem context is loaded from (empty where the step needs none)
//   load(src, b)        -> the per-problem context of problem b, handed to step
//   step(tot, h, ctx, next, len2) -> false = singular, else the next pose and the squared length of the move, as the path measures it
//   src, pass(st, grid, geom, B, poses, pose_stride, done, part): host side -- the value of Src and the launch of the path's pass kernel on grid one-wave workgroups
// The text below is instantiated in each translation unit with that unit's flags: it rounds as the file that includes it rounds.
#pragma once
#include "kernels.h"
#include "dmath.h"
#include "../../include/dsac_hip.h"

namespace dk {

DM_INLINE bool finite_d(double v) { return v - v == 0.0; }

// one wave per workgroup: its LDS operations execute in order, so a wave barrier (no counter wait: global loads may stay in flight) is all that separates
// a write from its readers
DM_INLINE void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

enum { SOFT_CONVERGED = 0, SOFT_MAXIT = 1, SOFT_SCORE = 2, SOFT_FEW = 3, SOFT_SINGULAR = 4, SOFT_NONFINITE = 5 };
static_assert(SOFT_CONVERGED == DSAC_SOFT_CONVERGED && SOFT_MAXIT == DSAC_SOFT_MAXIT && SOFT_SCORE == DSAC_SOFT_SCORE && SOFT_FEW == DSAC_SOFT_FEW &&
                  SOFT_SINGULAR == DSAC_SOFT_SINGULAR && SOFT_NONFINITE == DSAC_SOFT_NONFINITE,
              "the loop's statuses are enum dsac_soft_status");

constexpr int SOFT_STATE = 16;  // doubles per problem between the launches of the split form: pose (6), trial pose (6), S, 3 unused

// scratch of a loop with nacc sums per pass: per-chunk sums | state | done | iters; soft_loop_bytes is where a caller's own records may follow
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t soft_off_state(int nacc, int B, const SoftGeom& g) { return align256((size_t)B * g.nchunks * nacc * 8); }
inline size_t soft_off_done(int nacc, int B, const SoftGeom& g) { return soft_off_state(nacc, B, g) + align256((size_t)B * SOFT_STATE * 8); }
inline size_t soft_off_iters(int nacc, int B, const SoftGeom& g) { return soft_off_done(nacc, B, g) + align256((size_t)B * 4); }
inline size_t soft_loop_bytes(int nacc, int B, const SoftGeom& g) { return soft_off_iters(nacc, B, g) + align256((size_t)B * 4); }

// the frame of problem b: frame_of[b], or b / per_frame (per_frame 0: frame 0), never trusted beyond the batch; wave-uniform
DM_INLINE int soft_problem_frame(int frames, const int32_t* frame_of, int per_frame, int b) {
    if (frames <= 1) return 0;
    const int f = frame_of ? frame_of[b] : (per_frame > 0 ? b / per_frame : 0);
    return uniform_frame(min(max(f, 0), frames - 1));
}

// the chunk sums of problem b added in index order: lane l < NACC adds value l; the totals in s_tot (LDS) for every lane
template <int NACC>
DM_INLINE void soft_ordered_sum(const double* __restrict__ part, int b, int nchunks, double* s_tot) {
    const int lane = threadIdx.x & 63;
    if (lane < NACC) {
        const double* p = part + (size_t)b * nchunks * NACC + lane;
        double v = 0.0;
        for (int ck = 0; ck < nchunks; ck++) v += p[(size_t)ck * NACC];
        s_tot[lane] = v;
    }
    wave_lds_sync();
}

// One decision of the loop, after the pass at `trial` gave tot[]: -1 = go on (h, S, it updated, trial = the next pose to take a pass at), else the status
// (h, S, it are the problem's output).  first: the pass at the start pose.  The same bits in every lane.
template <class POLICY, class CTX>
DM_INLINE int soft_decide(bool first, const double* tot, const CTX& ctx, double h[6], double trial[6], double& S, int& it, double min_soft, int max_iters,
                          double step_tol) {
    const double Sn = tot[POLICY::S_AT];
    if (first) {
        bool finite = true;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            h[i] = trial[i];
            finite = finite && finite_d(trial[i]);
        }
        it = 0;
        S = finite ? Sn : 0.0;
        if (!finite) return SOFT_NONFINITE;
        if (!(Sn >= min_soft)) return SOFT_FEW;
    } else {
        if (!(Sn >= S)) return SOFT_SCORE;
        S = Sn;
        it++;
#pragma unroll
        for (int i = 0; i < 6; i++) h[i] = trial[i];
        if (it >= max_iters) return SOFT_MAXIT;
    }
    double next[6], len2;
    if (!POLICY::step(tot, h, ctx, next, len2)) return SOFT_SINGULAR;
    double den = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) den += h[i] * h[i];
    if (sqrt(len2) <= step_tol * (sqrt(den) + 2.220446049250313e-16)) return SOFT_CONVERGED;
#pragma unroll
    for (int i = 0; i < 6; i++) trial[i] = next[i];
    return -1;
}

DM_INLINE void soft_write_result(int b, int status, const double h[6], double S, int it, double* __restrict__ out_poses, double* __restrict__ soft_out,
                                 int32_t* __restrict__ iters_out, int32_t* __restrict__ status_out) {
#pragma unroll
    for (int i = 0; i < 6; i++) out_poses[(size_t)b * 6 + i] = h[i];
    if (soft_out) soft_out[b] = S;
    if (iters_out) iters_out[b] = it;
    if (status_out) status_out[b] = status;
}

// split form, the step: one wave per problem adds the pass's chunk sums in index order, decides and moves the pose
template <class POLICY>
__global__ __launch_bounds__(64) void k_soft_step(int B, int first, const double* __restrict__ init_poses, const double* __restrict__ part, int nchunks,
                                                  typename POLICY::Src src, double* __restrict__ state, int32_t* __restrict__ done, int32_t* __restrict__ iters,
                                                  double min_soft, int max_iters, double step_tol, double* __restrict__ out_poses, double* __restrict__ soft_out,
                                                  int32_t* __restrict__ iters_out, int32_t* __restrict__ status_out) {
    const int b = blockIdx.x;
    if (b >= B) return;
    if (!first && done[b]) return;
    const int lane = threadIdx.x & 63;
    __shared__ double s_tot[POLICY::NACC];
    soft_ordered_sum<POLICY::NACC>(part, b, nchunks, s_tot);
    const auto ctx = POLICY::load(src, b);
    double* st = state + (size_t)b * SOFT_STATE;
    double h[6], trial[6], S = 0.0;
    int it = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        trial[i] = first ? init_poses[(size_t)b * 6 + i] : st[6 + i];
        h[i] = first ? trial[i] : st[i];
    }
    if (!first) { S = st[12]; it = iters[b]; }
    const int status = soft_decide<POLICY>(first != 0, s_tot, ctx, h, trial, S, it, min_soft, max_iters, step_tol);
    if (lane != 0) return;
    if (status >= 0) {
        soft_write_result(b, status, h, S, it, out_poses, soft_out, iters_out, status_out);
        done[b] = 1;
        return;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) { st[i] = h[i]; st[6 + i] = trial[i]; }
    st[12] = S;
    iters[b] = it;
    if (first) done[b] = 0;
}

// split form, the host loop: max_iters + 1 pass and step launches, no round trip.  Pass k is taken at the start pose (k = 0) or at the trial pose the step
// before it wrote; finished problems return after one flag load
template <class POLICY>
hipError_t soft_loop(hipStream_t st, const POLICY& pol, int B, const double* init_poses, double min_soft, int max_iters, double step_tol, const SoftGeom& geom,
                     void* scratch, double* out_poses, double* soft_out, int32_t* iters_out, int32_t* status_out) {
    char* s = static_cast<char*>(scratch);
    double* part = reinterpret_cast<double*>(s);
    double* state = reinterpret_cast<double*>(s + soft_off_state(POLICY::NACC, B, geom));
    int32_t* done = reinterpret_cast<int32_t*>(s + soft_off_done(POLICY::NACC, B, geom));
    int32_t* iters = reinterpret_cast<int32_t*>(s + soft_off_iters(POLICY::NACC, B, geom));
    const unsigned grid = (unsigned)B * (unsigned)geom.nchunks;
    for (int k = 0; k <= max_iters; k++) {
        pol.pass(st, grid, geom, B, k == 0 ? init_poses : state + 6, k == 0 ? 6 : SOFT_STATE, k == 0 ? (const int32_t*)nullptr : done, part);
        hipLaunchKernelGGL(k_soft_step<POLICY>, dim3((unsigned)B), dim3(64), 0, st, B, k == 0 ? 1 : 0, init_poses, part, geom.nchunks, pol.src, state, done, iters,
                           min_soft, max_iters, step_tol, out_poses, soft_out, iters_out, status_out);
    }
    return hipGetLastError();
}

}  // namespace dk
