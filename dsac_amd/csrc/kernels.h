// kernels.h -- host-callable launchers of the gfx950 kernels (one .hip translation unit per group).
// All pointers are DEVICE pointers; every launcher only enqueues work on `st` and returns the HIP status
// of the last launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k2_plan.h"

namespace dk {

struct FrameDev {
    const float* xyz;  // P x 3 (mm)
    const float* uv;   // P x 2 or nullptr (implicit grid u = x, v = y)
    int H, W, P;
    float fx, fy, cx, cy;
    // frame batch (dsac_set_frames): `frames` maps of the same geometry back to back, frame f at xyz + f * xyz_stride
    // (floats); uv is shared (uv_stride == 0) or per frame.  Only K1 (random sampling), K2 and K3 look at frames > 0.
    int frames = 1;
    long long xyz_stride = 0, uv_stride = 0;
    int seed_stride = 1;  // frame f of a batch draws from the random stream of seed + f * seed_stride (dsac_set_option "seed_stride")
    // one camera per frame (dsac_set_frames_cams): frames x (fx, fy, cx, cy) in device memory the context owns, nullptr = the shared camera above.
    // fx .. cy then hold row 0 until a kernel selects its frame (select_frame); cams_h is the context's host copy of the same rows, for the code that
    // walks a batch frame by frame on the host (frame_cam) -- no kernel reads it
    const float4* cams = nullptr;
    const float* cams_h = nullptr;
};

// The frame selection of every kernel that is handed a whole batch: xyz / uv move to frame `frame`, and with per-frame cameras the frame's row replaces
// fx .. cy, so that make_cam / make_cam_r and everything behind them see the frame's own camera.  `frame` is wave-uniform at every call site (a workgroup or
// a wave owns one hypothesis / problem / list); sites where the compiler cannot see that pass it through uniform_frame, which keeps the row a scalar load.
__device__ __forceinline__ void select_frame(FrameDev& F, long long frame) {
    F.xyz += frame * F.xyz_stride;
    if (F.uv) F.uv += frame * F.uv_stride;
    if (F.cams) {
        const float4 k = F.cams[frame];
        F.fx = k.x; F.fy = k.y; F.cx = k.z; F.cy = k.w;
    }
}
__device__ __forceinline__ int uniform_frame(int frame) { return __builtin_amdgcn_readfirstlane(frame); }
// the same selection on the host, for a FrameDev that stands for frame f alone (the caller has moved xyz / uv): the camera from the host copy, no table
inline void frame_cam(FrameDev& G, int f) {
    if (G.cams_h) { G.fx = G.cams_h[4 * f]; G.fy = G.cams_h[4 * f + 1]; G.cx = G.cams_h[4 * f + 2]; G.cy = G.cams_h[4 * f + 3]; }
    G.cams = nullptr;
    G.cams_h = nullptr;
}

// Staged pose record used by K2, 12 floats (48 B, three float4 rows) per hypothesis:
//   [0..3]  fx*R0 | fx*tx      [4..7] fy*R1 | fy*ty      [8..11] R2 | tz
constexpr int POSE_STRIDE = 12;

// ---- k_forward.hip ---------------------------------------------------------------------------------
// fp64 Rodrigues of N cv poses -> staged float records.
// Nf (per-frame cameras): hypotheses per frame, hypothesis h folds the camera of frame h / Nf; 0 = one frame
hipError_t pose_prep(hipStream_t st, int N, const double* poses, const FrameDev& F, float* staged, int Nf = 0);
hipError_t pose_prep_lo(hipStream_t st, int N, const double* poses, const FrameDev& F, float* staged_lo, int Nf = 0);  // what the float records leave behind
// the records of the exact-transform form (k2_flags bit 28): pose_split_bytes(N) bytes; available for focal lengths up to 2^10 (pose_split_exponent <= 10)
size_t pose_split_bytes(int N);
int pose_split_exponent(const FrameDev& F);
bool pose_split_available(const FrameDev& F);
hipError_t pose_prep_split(hipStream_t st, int N, const double* poses, const FrameDev& F, void* split, int Nf = 0);

// K2.  err (N x P) and/or soft partials.  soft_part must hold reproject_num_pixel_tiles(P) * N floats.
// The knobs (K2Opts), the flags and the decision which kernel runs (k2_plan) are in k2_plan.h; reproject() enqueues the kernel of a plan whose status is
// K2_STATUS_OK and decides nothing.  N, F, err and soft_part are the ones the plan was made for (soft_part non-NULL exactly when the plan writes sums).
// What a launch is handed per call: the records the plan names, the cv poses, the timing events, "k2_diag"
struct K2Call {
    const float* staged_lo = nullptr;  // the low parts of the staged records (pose_prep_lo), where the plan says need_lo
    const void* split = nullptr;       // the split fp16 records (pose_prep_split), where the plan says need_split
    const double* poses64 = nullptr;   // the cv poses (N x 6 doubles) the staged records were made from -- the precise form works from these
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;  // timing events attached to the K2 dispatch itself (profiling), else null
    int diag = 0;
};
hipError_t reproject(hipStream_t st, const K2Plan& plan, int N, const float* staged, const FrameDev& F, float clampv, float* err, float tau, float beta,
                     float* soft_part, const K2Call& call);
// soft[h] = sum over pixel tiles of soft_part[tile][h]   (double, deterministic)
hipError_t reduce_soft(hipStream_t st, int N, int tiles, const float* soft_part, double* soft);
// what the exact form degrades on (dsac_k2_range_census): out[0] += 64-cell chunks of the frame(s) with a coordinate outside the split's range (split_B's
// predicate: those chunks take the fp32 transform), out[1] += hypotheses whose split records clamp a piece or hold a non-finite entry.  One small kernel.
hipError_t k2_range_census(hipStream_t st, int N, const double* poses, const FrameDev& F, unsigned long long* out2, int Nf = 0);
// K3.
// frames > 1: one independent softmax per consecutive group of N scores (outputs entropy[frames], avg6[frames][6])
hipError_t softmax(hipStream_t st, int N, const double* scores, double scale, double* w, double* entropy, const double* poses, double* avg6,
                   int frames = 1);

// ---- k_sample.hip ----------------------------------------------------------------------------------
// Nf > 0 (frame batch): hypothesis h belongs to frame h / Nf and draws from the stream of (seed + frame, h % Nf), i.e. exactly
// what a single-frame call with seed + frame would draw.
// Launch knobs of K1 (context state like K2Opts): waves per workgroup (DSAC_K1_WPB in {1, 4, 8}), wave priority (DSAC_K1_PRIO 0..3),
// hypotheses per wave (DSAC_K1_HPW in {1, 2, 4}), OpenCV's Jacobi sweeps for the alignment of the P3P triangle instead of the closed form (DSAC_K1_HORN).
// Guided sampling: what the table build records per frame next to the table itself.
struct GuideMeta {
    uint64_t T;      // total mass = C_f[P - 1]
    double S;        // sum of the valid weights (double), for the score-function gradient
    uint32_t wmax;   // bits of the largest valid weight (positive floats order like their bits), 0 = no valid cell
    int32_t n;       // cells with mass > 0
};
// what a guided draw reads of a built table (2D or RGB-D; the context owns the buffers): frames x P inclusive sums of the quantised masses, the per-frame
// records, and the coarse level, frames x guide_coarse_entries(P)
struct GuideView { const uint64_t* cdf; const GuideMeta* meta; const uint64_t* coarse; };
// the coarse level of a frame's table: the last entry of every block of 2^shift cells, the smallest shift >= 8 that leaves at most GUIDE_COARSE_MAX blocks
// (K1 keeps them in LDS: 16 KB; 640x480 is 1 200 blocks of 256)
constexpr int GUIDE_COARSE_MAX = 2048;
__host__ __device__ inline int guide_coarse_shift(int P) {
    int s = 8;
    while (((P + (1 << s) - 1) >> s) > GUIDE_COARSE_MAX) s++;
    return s;
}
__host__ __device__ inline int guide_coarse_entries(int P) { const int s = guide_coarse_shift(P); return (P + (1 << s) - 1) >> s; }
constexpr int GUIDE_TILE = 1024;  // cells per workgroup of the table build (256 lanes x 4 consecutive cells)
inline int guide_tiles(int P) { return (P + GUIDE_TILE - 1) / GUIDE_TILE; }
// scratch of a build: per frame and tile the tile's mass (uint64), its valid-weight sum (double) and its count of cells with mass (uint64)
inline size_t guide_scratch_bytes(int frames, int P) { return (size_t)frames * guide_tiles(P) * 24; }
// The table build, a few small launches on st: the valid maximum per frame, the masses m_p = floor((double) w_p / (double) wmax * 2^24) and their tile sums, the
// scan of the tile sums (which records T, n and S), the inclusive uint64 scan.  w: frames x P floats (device); w_copy: the context's copy of them (the build's
// first launch writes it; every later launch reads the copy, so the caller may overwrite w in stream order)
hipError_t guide_build(hipStream_t st, int frames, int P, const float* w, float* w_copy, uint64_t* cdf, uint64_t* coarse, GuideMeta* meta, void* scratch);
// grad_w[f * P + p] += sum over the accepted hypotheses h of frame f of g[h] * ([p in set_h] / w_p - set_cells / S_f), valid cells only; one launch.
// set_cells: cells per minimal set, 4 (sets N x 4) or 3 (the RGB-D sets, N x 3)
hipError_t guide_backward(hipStream_t st, int frames, int P, int Nf, const float* w_copy, const GuideMeta* meta, const int32_t* sets, const uint8_t* ok,
                          const double* g, double* grad_w, int set_cells = 4);
struct K1Opts {
    int wpb = 1, prio = 3, hpw = 1, minw = 1;  // minw: minimum waves per SIMD of the register allocation (DSAC_K1_MINW)
    bool share_always = false;  // share beyond 1024 hypotheses as well (DSAC_K1_SHARE < 0)
    int share = 4;  // waves of a workgroup that help each other's unfinished hypotheses (k_sample_shared; 0 / 1 = off, 4, 8; DSAC_K1_SHARE)
    bool horn = false;
    int wide = -1;  // waves per hypothesis of the one-lane-per-attempt form for few hypotheses: -1 auto (2 up to 512 hypotheses), 0 off, 2, 4 (4: up to 256) (DSAC_K1_WIDE)
    int rl = 1;  // lanes per attempt: 4 = one per quartic root, 1 = one lane per attempt with its roots in sequence (DSAC_K1_RL)
};
// guide: the context's table while sampling weights are active (dsac_set_sampling_weights), else nullptr.  sample() then launches the guided build (one lane
// per attempt, one hypothesis per wave) whatever the form knobs say -- they never change a result -- and given sets ignore it
hipError_t sample(hipStream_t st, int N, uint64_t seed, const int32_t* sets_in, const FrameDev& F, int thr_int, int max_tries,
                  double* poses, int32_t* sets_out, uint8_t* ok, float* staged_or_null = nullptr, int Nf = 0,
                  const K1Opts& opts = K1Opts(), const GuideView* guide = nullptr);  // staged: K2 records (N x 12)
// K1 in the reference's own random stream (round 6; core/thread_rand.cpp:40-69, core/cnn_softam.h:1010-1060; refstream.h): T generators std::mt19937(seed + t)
// on the device; a window = A attempts per stream parsed, evaluated and handed to the stream's next hypotheses in order.
struct RefStreamState { uint32_t mt[624]; uint32_t idx; uint32_t pad[3]; };
constexpr int refstream_window_outputs(int A) { return 9 * A + 128; }  // raw outputs generated per window (an attempt takes 8, rarely more)
size_t refstream_window_bytes(int T, int A);
hipError_t refstream_init(hipStream_t st, RefStreamState* states, uint32_t seed, int T);
hipError_t refstream_discard(hipStream_t st, RefStreamState* states, int t, unsigned long long n);
// first / served / need / parsed [T] int32, consumed [T] uint64, attempts [T] int64: device arrays (served / need / consumed / attempts are updated)
hipError_t refstream_window(hipStream_t st, RefStreamState* states, int T, int A, int mode, void* scratch, const FrameDev& F, int thr_int, const int32_t* first,
                            int32_t* served, int32_t* need, int32_t* parsed, unsigned long long* consumed, long long* attempts, double* poses, int32_t* sets_out,
                            uint8_t* ok, float* staged);
// the same loop as an enqueue-only chain over the images of a frame batch, window sizes fixed beforehand (rs::window_ladder); scratch holds
// refstream_window_bytes(T, largest window), small 3 T int32 + T uint64 + T int64
hipError_t refstream_chain(hipStream_t st, RefStreamState* states, int T, int N, int frames, const int* windows, int n_windows, int mode, void* scratch, void* small,
                           const FrameDev& F, int thr_int, unsigned long long discard0, double* poses, int32_t* sets_out, uint8_t* ok, float* staged,
                           unsigned long long* consumed_or_null, long long* attempts_or_null);
hipError_t refstream_unserved(hipStream_t st, int T, const int32_t* first, const int32_t* served, const int32_t* need, const FrameDev& F, double* poses, int32_t* sets_out,
                              uint8_t* ok, float* staged);
// Nf (frame batch): hypotheses per frame, hypothesis h reads frame h / Nf
hipError_t dpnp(hipStream_t st, int N, const int32_t* sets, const FrameDev& F, float eps, double* J, int Nf = 0);

// ---- k_backward.hip --------------------------------------------------------------------------------
// jp-convention staged records for the backward pass, BWD_STRIDE floats per hypothesis (see k_backward.hip).
constexpr int BWD_STRIDE = 24;  // six float4 per hypothesis, already sign-folded and pair-packed for K4's packed-fp32 chains
// Launch plan of the K4 main pass: which kernel form, its hypothesis tile and the sizes of the two partial-sum buffers.
//   variant 0 = VALU form (lane = 8 pixels, wave reduction of the 12 sums per hypothesis), 1 .. 5 = matrix-core form with 2 / 4 / 5 / 6 / 3 16-pixel
//   chunks per wave (lane = one hypothesis x 4 consecutive pixels), -1 = auto.  Maps that cannot be read as 16-byte vectors use variant 0.
struct K4Plan {
    int variant;  // resolved form
    int HT, NT;   // hypotheses per workgroup, number of hypothesis tiles (rows of grad_part)
    int rows;     // rows of G12_part the launch writes
    int glayers;  // layers of grad_part per hypothesis tile (matrix-core form: 2 -- a pixel tile's hypothesis groups may be split between two workgroups)
    bool fused = false;   // round 4: no backward_prep launch -- the main pass derives its records from the poses, the finish kernel dR/drod; G12_part [hyp][row][12]
    bool direct = false;  // ... and (one hypothesis tile) the main pass adds its gradient straight into grad_xyz: no grad_part, no gradient reduction launch
    int Nf = 0;           // frame batch: hypotheses per frame (= HT), 0 = one frame
    int elem = 0;         // element type of d_err (K4_ELEM_*); K4_ELEM_F16 / K4_ELEM_BF16: N x P IEEE binary16 / bfloat16, the matrix-core form only (variant > 0, not the soft mode)
};
enum { K4_ELEM_F32 = 0, K4_ELEM_F16 = 1, K4_ELEM_BF16 = 2 };
// the bfloat16 build of the matrix-core form exists where it needs no scratch: forms 1, 2 and 5 (2, 4 and 3 chunks at two waves per SIMD -- what the auto plan
// picks, and the 3-chunk knob).  The 5- and 6-chunk forms (3, 4) and the high-occupancy forms (6, 7) spill in every element type and are not built in bfloat16
inline bool k4_form_has_bf16(int form) { return form == 1 || form == 2 || form == 5; }
// Nf > 0 (frame batch): N = frames x Nf hypotheses, one hypothesis tile per frame (Nf a multiple of 16, <= 256), gradient per frame (grad_xyz frames x P x 3);
// plan.variant == 0 then means: not available for a batch
// elem: what d_err points to (K4_ELEM_*).  The half plan is the float plan -- same variant, tiles, rows, fused / direct -- with d_err on an 8-byte address
// where the float plan wants 16; variant 0 (the VALU form) does not read halves: the caller refuses
K4Plan backward_plan(int N, const FrameDev& F, const void* d_err, int variant, int Nf = 0, int elem = K4_ELEM_F32);
bool backward_variant_known(int variant);  // -1 (auto), 0 .. 5, or a form + 10 * tile code + 100 * workgroups per CU (see backward_plan)
constexpr int BWD_DRDH = 54;  // per hypothesis: dR/drod (27) and Omega_i = (dR/drod_i) R^T (27)
hipError_t backward_prep(hipStream_t st, int N, const double* poses, const FrameDev& F, float* staged_bwd, double* dRdH /*N x BWD_DRDH*/);
// K4 main pass.  d_err (N x P floats, or 16-bit elements with plan.elem == K4_ELEM_F16 / K4_ELEM_BF16) or nullptr with g (N doubles) for the soft-inlier score.
//   grad_part : [hyp_tiles][P*3] floats       G12_part : [partial rows][N][12] floats
// poses (cv, N x 6) / grad_xyz (P x 3 fp64, accumulated into) / flags: used when plan.fused / plan.direct (staged_bwd and grad_part may then be nullptr)
hipError_t score_backward(hipStream_t st, int N, const float* staged_bwd, const FrameDev& F, const void* d_err, const double* g,
                          float clampv, float tau, float beta, float* grad_part, float* G12_part, const K4Plan& plan, const double* poses = nullptr,
                          double* grad_xyz = nullptr, unsigned flags = 0);
// Epilogue: grad_xyz (P x 3 double) += sum over hyp tiles; then per hypothesis G6 = [G9 * dRdH, G3],
// S = G6 * dPNP_h, scatter-add S to the 4 support pixels.
hipError_t score_backward_finish(hipStream_t st, int N, const FrameDev& F, const float* grad_part, int hyp_tiles, const float* G12_part,
                                 int pixel_tiles, const double* dRdH, const double* dpnp, const int32_t* sets, unsigned flags,
                                 double* grad_xyz, double* G6_scratch, const float* rec_if_e_based = nullptr, const double* poses_if_fused = nullptr, int Nf = 0);
// hyp_tiles == 0: no gradient reduction (plan.direct); poses_if_fused: the cv poses when plan.fused (dRdH and rec_if_e_based are then unused)
// rec_if_e_based: the BWD records when G12_part holds the matrix-core form's E-based sums (K4Plan.variant > 0), else nullptr
// K4 parity mode (fp64, the reference's evaluation order; flags bit 0 = transposed columns, bit 2 = rotation write-back); jac_scratch: N x P*3 doubles
hipError_t score_backward_parity(hipStream_t st, int N, const double* poses, const FrameDev& F, const float* d_err, const double* dpnp, const int32_t* sets,
                                 unsigned flags, double* jac_scratch, double* grad_xyz, double* G6_out);
// frames > 1: N hypotheses PER FRAME, v6 frames x 6, grad_xyz frames x P x 3, one workgroup per frame
hipError_t path1_softmax_backward(hipStream_t st, int N, int P, const double* v6, const double* w, const double* poses, const int32_t* sets,
                                  const double* dpnp, double* grad_xyz, double* g, double g_scale = 1.0, int frames = 1);
// grad[obj_pixels[i]] += dL . J_obj[i] for i < min(*n_obj, cap), v6 = dL . J_hyp
// frames > 1: every array holds one slice per frame (dL 6, J_hyp 36, obj_pixels px_stride, J_obj cap*18, n_obj 1, grad_xyz P*3, v6 6)
hipError_t path1_assemble(hipStream_t st, const double* dL, const double* J_hyp, const int32_t* obj_pixels, const double* J_obj, const int32_t* n_obj,
                          int cap, int P, double* grad_xyz, double* v6, int frames = 1, int px_stride = 0);

// ---- k_refine.hip ----------------------------------------------------------------------------------
// inlier_map: map_stride == 0 -> H*W counters of problem 0 only; map_stride == H*W -> one map per problem
// per_frame > 0 (frame batch): problem b refines against frame b / per_frame (F.xyz_stride / F.uv_stride)
hipError_t refine(hipStream_t st, int B, const double* init_poses, const int32_t* perm, int steps, int max_inl, int min_inl, float thr,
                  const int32_t* pert_px_c, const float* pert_value, const FrameDev& F, double* out_poses, int32_t* inlier_map,
                  int32_t* steps_done, int map_stride = 0, int per_frame = 0, const double* loss_gt_jp6 = nullptr, double* loss_out4 = nullptr,
                  int waves_per_problem = 0);
// many problems with long walks (the DSAC variant on big maps): a refinement step as two launches, a scan of the step's pre-permuted cells + LM (k_refine.hip); the
// same results bit for bit.  refine_split_applies: >= 32 problems, >= 16 384 cells, no perturbation, no fused loss, "k6_waves" 0
size_t refine_split_scratch_bytes(int B, int steps, int frames, int P, int max_inl);
void refine_scan_tune(int v);  // experiments ("k6_scan_tune")
int refine_scan_tune_get();   // the value last set
bool refine_split_applies(int B, const FrameDev& F, const int32_t* pert_px_c, const double* loss_out4, int waves_per_problem);
hipError_t refine_split(hipStream_t st, int B, const double* init_poses, const int32_t* perm, int steps, int max_inl, int min_inl, float thr, const FrameDev& F,
                        double* out_poses, int32_t* inlier_map, int32_t* steps_done, int map_stride, int per_frame, void* scratch, int exact_only = 0);
// exact_only ("k6_walk_exact"): the walk's fp32 filter off -- every cell by the fp64 residual (A/B; the decisions are the same)
// waves_per_problem: 0 = by the problem count (1 for a single problem, 4 up to 512 problems, 2 up to 1 024, else 1), 1 / 2 / 4 / 8 = fixed ("k6_waves"); the same results bit for bit
// loss_gt_jp6 (B x 6) / loss_out4 (B x 4): maxLoss of every refined pose against its ground truth in the same launch (K7's arithmetic, loss_math.h)
// inlier_maps[h][set cell] = 0 for the 4 cells of every hypothesis' minimal set (core/cnn.h:1208-1214)
hipError_t zero_set_cells(hipStream_t st, int N, const int32_t* sets, int P, int32_t* inlier_maps);
// ---- K6's finite-difference Jacobians: plan the replica lists, run the replicas through k_refine, central differences ----
// A batch of replica lists.  head = FD_HEAD_POSE: dRefineHyp + dRefineObj (core/cnn_softam.h), 12 replicas perturb the given start pose, one list per frame.
// head = FD_HEAD_SET: the DSAC variant (core/cnn.h:854-990 dRefine), 18 replicas perturb the first three points of the minimal set and every replica's start
// pose is P3P of the set read from the perturbed map, one list per hypothesis.  6 replicas per selected inlier cell follow in both.
constexpr int FD_HEAD_POSE = 12, FD_HEAD_SET = 18;
struct FdLists {
    int head;                 // head replicas per list
    int lists;                // list m: replicas() entries of the replica arrays, its own inlier map (H*W), n_obj[m], cap x 18 of J_obj
    int cap;                  // at most cap selected cells per list
    int px_stride;            // obj_pixels of list m at m * px_stride
    bool list_is_frame;       // list m reads frame m of the batch (FD_HEAD_POSE only) ...
    const int32_t* frame_of;  // ... else frame frame_of[m] (lists int32, device), nullptr: the single frame
    int replicas() const { return head + 6 * cap; }
};
struct FdReplicas {  // lists x replicas() each: start poses (x 6), perturbed cell and channel (x 2; cell -1: none), perturbed value, refined poses (x 6)
    double* poses;
    int32_t* px_c;
    float* value;
    double* out;
};
// scratch of the plan per list: int32 of device memory (0: small map, one workgroup per list scans it) -- large maps are planned by two tiled launches
size_t refine_fd_plan_scratch_ints(const FrameDev& F);
// init_pose: lists x 6 (FD_HEAD_POSE), set4: lists x 4 (FD_HEAD_SET), the other one unused; eps_hyp: FD_HEAD_POSE only
hipError_t refine_fd_plan(hipStream_t st, const FdLists& L, const double* init_pose, const int32_t* set4, const int32_t* inlier_map, const FrameDev& F, int skip,
                          float eps_hyp, float eps_obj, const FdReplicas& rep, int32_t* obj_pixels, int32_t* n_obj, int32_t* scratch);
// one launch of lists x replicas() waves; those beyond head + 6 * n_obj[m] of their list exit immediately
hipError_t refine_fd_run(hipStream_t st, const FdLists& L, const int32_t* n_obj, const int32_t* perm, int steps, int max_inl, int min_inl, float thr,
                         const FrameDev& F, const FdReplicas& rep);
// J_head: lists x 6 x 6 (J_hyp; rows 3-5 over 2 eps_hyp * 1000) or lists x 6 x 9 (J_set, over 2 eps_obj); J_obj over 2 eps_obj, scaled by skip
hipError_t refine_fd_finish(hipStream_t st, const FdLists& L, const double* rep_out, const int32_t* n_obj, int skip, float eps_hyp, float eps_obj, double* J_head,
                            double* J_obj);
// ---- K6's analytic backward: the Gauss-Newton linearisation of a refined pose (dsac_refine_gn_backward, include/dsac_hip.h), one launch of B waves ----
// problem b: pose ref_poses[b] (cv), frame frame_of[b] (clamped) or b / per_frame (per_frame 0: frame 0), permutation row rows[b] (clamped; nullptr: row 0).
// grad_xyz (frames x P x 3, accumulated with fp64 atomics) needs dL (B x 6, jp); coef nullptr = 1.  cells B x max_inl, J_obj B x max_inl x 6 x 3, n_out B.
// A problem without a result (fewer than min_inl cells, a non-finite pose, a non-positive pivot) writes n_out[b] = 0 and nothing else.
hipError_t refine_gn(hipStream_t st, int B, const double* ref_poses, const int32_t* frame_of, int per_frame, const int32_t* perm, int steps, const int32_t* rows,
                     int max_inl, int min_inl, float thr, const double* dL, const double* coef, double* grad_xyz, int32_t* cells, double* J_obj, int32_t* n_out,
                     const FrameDev& F);
// ---- soft-inlier refinement over the whole map (dsac_refine_soft / dsac_refine_soft_backward, include/dsac_hip.h) ----
// chunk geometry of the split form's passes: computed once per call (it depends on the map alone) and handed to the scratch sizing and to the launch
struct SoftGeom { int chunk, nchunks; };
SoftGeom refine_soft_geom(int P);
size_t refine_soft_scratch_bytes(int B, const SoftGeom& g);
bool refine_soft_auto_fused(int P);  // what "refine_soft_form" -1 takes
// fused: one launch of B workgroups; else max_iters + 1 pass and step launches.  soft_out / iters_out / status_out may be nullptr.  Problem b: frame frame_of[b]
// (clamped) or b / per_frame (per_frame 0: frame 0)
hipError_t refine_soft(hipStream_t st, int B, const double* init_poses, const int32_t* frame_of, int per_frame, double tau, double beta, double cut, double min_soft,
                       int max_iters, double step_tol, bool fused, const SoftGeom& geom, void* scratch, double* out_poses, double* soft_out, int32_t* iters_out,
                       int32_t* status_out, const FrameDev& F);
// pass (H_b), solve (q_b), scatter (a lane per cell, the frame's problems in index order): three launches, no atomics.  flags bit 0: fixed weights
hipError_t refine_soft_backward(hipStream_t st, int B, const double* ref_poses, const int32_t* frame_of, int per_frame, double tau, double beta, double cut,
                                double min_soft, const double* dL, const double* coef, unsigned flags, const SoftGeom& geom, void* scratch, double* grad_xyz,
                                int32_t* ok_out, const FrameDev& F);

// ---- k_loss.hip ------------------------------------------------------------------------------------
// gt_stride: 0 = one ground truth (6 doubles) for all estimates, 6 = one per estimate
// gt_group: estimates b share the ground truth of index b / gt_group (a frame batch of the DSAC variant: N estimates per frame)
hipError_t pose_loss(hipStream_t st, int B, const double* est_cv6 /*B x 6*/, const double* gt_jp6, double* out4 /*B x 4*/, double* J6 /*B x 6*/,
                     int gt_stride = 0, int gt_group = 1);

// DSAC variant: draw (core/cnn.h:102-127; u < 0: argmax), expectedMaxLoss (:137-150), the score gradients of dSMScore (:737-742); losses[i * loss_stride]
hipError_t dsac_select(hipStream_t st, int N, const double* w, const double* losses, int loss_stride, double u, double eps, int32_t* hyp_idx, double* expected,
                       double* g);
// the same for `frames` images in one launch (a workgroup per image): w / losses / g [frames][N], u / hyp_idx / expected [frames]; u on the device
hipError_t dsac_select_frames(hipStream_t st, int frames, int N, const double* w, const double* losses, int loss_stride, const double* u, double eps,
                              int32_t* hyp_idx, double* expected, double* g);

// ---- k_patches.hip ---------------------------------------------------------------------------------
// n patches of 3 x patch x patch floats (patch, channel, row, column) around sampling_xy[i] = (x, y) of an H x W x 3 BGR image
hipError_t gather_patches(hipStream_t st, const uint8_t* bgr, int H, int W, const int32_t* sampling_xy, int n, int patch, float* out, int32_t* skipped);

// ---- k_rgbd.hip ------------------------------------------------------------------------------------
// RGB-D localisation (dsac_set_camera_points / dsac_sample_rgbd / dsac_score_rgbd / dsac_refine_rgbd, include/dsac_hip.h).  The measured camera-frame points
// travel as arguments of their own: cam = the context's canonical copy (frames x P x 3, NaN in all three components of a cell that is not VALID), meta = per
// frame the number of VALID cells and the first VALID cell (2 int32; 0x7fffffff: none).  No kernel of this group reads the camera intrinsics.
// two launches: meta's reset, then the copy that canonicalises, counts and finds the first VALID cell.  src: frames x P x 3 (device)
hipError_t rgbd_set_points(hipStream_t st, const float* src, const FrameDev& F, float* cam_copy, int32_t* meta);
// sets N x 3.  sets_in: evaluated once each (one frame); else drawn from K1's counter stream, Nf > 0: hypothesis h belongs to frame h / Nf
// guide: the table of dsac_set_sampling_weights_rgbd while those weights are active (drawn sets then come from it: the guided build), else nullptr
hipError_t rgbd_sample(hipStream_t st, int N, uint64_t seed, const int32_t* sets_in, const FrameDev& F, const float* cam, const int32_t* meta, double thr,
                       int max_tries, double* poses, int32_t* sets_out, uint8_t* ok, int Nf = 0, const GuideView* guide = nullptr);
// the masked weights of guided RGB-D sampling, one launch: out[f * P + p] = w[f * P + p] where the cell is VALID in the canonical copy, 0 elsewhere
hipError_t rgbd_mask_weights(hipStream_t st, int frames, int P, const float* w, const float* cam, float* out);
// rec: N x POSE_STRIDE floats (written here); err (N x P) and / or soft (N doubles; soft_part then holds rgbd_score_tiles(P) x N floats), either may be nullptr
int rgbd_score_tiles(int P);
hipError_t rgbd_score(hipStream_t st, int N, const double* poses, float* rec, const FrameDev& F, const float* cam, float clampv, float* err, float tau, float beta,
                      float* soft_part, double* soft, int Nf = 0);
// the split loop of refine_soft (soft_loop.h) with the RGB-D pass and step (chunks: refine_soft_geom)
size_t rgbd_refine_scratch_bytes(int B, const SoftGeom& g);
hipError_t rgbd_refine(hipStream_t st, int B, const double* init_poses, const int32_t* frame_of, int per_frame, double tau, double beta, double cut, double min_soft,
                       int max_iters, double step_tol, const SoftGeom& geom, void* scratch, double* out_poses, double* soft_out, int32_t* iters_out,
                       int32_t* status_out, const FrameDev& F, const float* cam, const int32_t* meta);

}  // namespace dk
