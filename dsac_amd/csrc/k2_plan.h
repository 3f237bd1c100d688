// k2_plan.h -- which K2 kernel scores a frame, decided on the host before anything is enqueued (as backward_plan() does for K4).
// No HIP in here: a plain C++ compiler builds it (tests/helpers/k2_plan_host.cpp walks it against tests/k2_plan_ref.py).
//   k2_plan(K2PlanIn) -> K2Plan : a refusal, or the arithmetic form, the kernel, the records it reads and the partial-sum rows it writes
//   dk::reproject() (k_forward.hip) launches a plan and decides nothing; k2_stage() (api.hip) asks for the plan first and builds what it names
// The size thresholds of the auto policy, the options under which only the exact form may run, and the list of k2_variant ids each stand here once.
#pragma once

namespace dk {

// Launch knobs of K2; they live in the context (read once from the environment in dsac_create, or set with dsac_set_option), never in process-wide state.
struct K2Opts {
    bool pixel_minor = true;  // block order: pixel tiles innermost (DSAC_K2_ORDER)
    int flags = 0;            // bit0: plain (cached) stores instead of non-temporal (DSAC_K2_FLAGS)
    int variant = -1;         // < 0 = auto policy, otherwise a fixed kernel form (DSAC_K2_VARIANT), see K2_FP32_IDS
    bool exact_auto = true;   // "k2_exact_auto" (DSAC_K2_EXACT_AUTO): the auto policy (variant -1, no other arithmetic flag) takes the exact-transform form wherever it
                              // applies -- round 6: the default K2 is the form that holds every stated tolerance; 0 = the fp32 matrix-core forms
    int diag = 0;             // "k2_diag": diagnostic switches of the precise form (which fp32 step costs what; k_reproject_prec), 0 = none; no part of the decision
    int f16_store = 1;        // "k2_f16_store": store layout of both 16-bit builds (binary16 and bfloat16): 0 = four 8-byte stores per lane and chunk, 1 (default: 882 against 892 us at the
                              // bench shape, profiles/k2_f16_ab.txt) = two 16-byte stores after a lane exchange
    int hyp_walk = 0;         // "k2_hyp_walk": hypothesis tiles a workgroup of the full-tile builds scores on its pixel tile: 0 = auto (k2_hyp_walk), 1 / 2 / 4 = that many
                              // wherever the kernel has the walk and no walk would straddle a frame or the end of N
};
enum { K2_ELEM_F32 = 0, K2_ELEM_F16 = 1, K2_ELEM_BF16 = 2 };
constexpr int K2_FLAG_STORE_ONLY = 1 << 1;  // k2_flags: store schedule only (measurement)
constexpr int K2_FLAG_ERR_UNFUSED = 1 << 24;  // k2_flags: an error-images-only call never takes the kernel with the sigmoid arithmetic (k2_fuse_sums; A/B)
constexpr int K2_FLAG_PRECISE = 1 << 25;  // k2_flags: the fp64 projection of the reference (k_reproject_prec) instead of the fp32 matrix-core transform
constexpr int K2_FLAG_REC32 = 1 << 26;    // k2_flags: the precise form on fp32 records (diagnosis)
constexpr int K2_FLAG_RECLO = 1 << 27;    // k2_flags: pose records in two pieces -- the low parts through fp16 matrix-core instructions chained onto the fp32 ones
constexpr int K2_FLAG_EXACT = 1 << 28;    // k2_flags: exact transform -- split fp16 records through the fp16 matrix core, the camera-frame point rounded to float once (round 6)
constexpr int K2_FLAG_EXACT_ANY = 1 << 29;  // k2_flags: the exact transform on whatever build fits the map (vector or any-map); an error only where the focal length rules the split records out
constexpr int K2_FLAG_GENERAL_PATH = 1 << 30;  // k2_flags: the exact vector builds take their general path on every tile, never the full-tile path (measurement: the A/B of the
                                                // two paths in one process); no part of the decision -- the form, the kernel and every result are the same with and without it
// what a launch computed with (dsac_get_option "k2_form_last"; the values of enum dsac_k2_form) and why it was not the exact form ("k2_form_why_last")
enum { K2_FORM_NONE = 0, K2_FORM_FP32_VALU = 1, K2_FORM_FP32_MFMA = 2, K2_FORM_RECLO = 3, K2_FORM_EXACT_VEC = 4, K2_FORM_EXACT_ANY = 5, K2_FORM_PRECISE = 6 };
enum { K2_WHY_AUTO_OFF = 1, K2_WHY_FORCED = 2, K2_WHY_FOCAL = 4, K2_WHY_NO_POSES = 8 };
// Nf of a frame batch must be a multiple of this: no hypothesis tile of any kernel form (<= 128 hypotheses) may straddle two frames
constexpr int K2_NF_MULTIPLE = 128;
constexpr int K2_KFLAG_WALK_SHIFT = 6;  // the kernels' flag bits 6-7: log2 of the plan's hyp_walk, put there by dk::reproject (never taken from "k2_flags")
constexpr int K2_WG = 256;  // threads per workgroup of the VALU, matrix-core and precise kernels (K2_THREADS)

// does a K2 launch with these options want the split records?  (bits 28 / 29 ask for them; the auto policy wants them unless another arithmetic form or a measurement flag is set)
inline bool k2_wants_exact(const K2Opts& o) {
    if (o.flags & (K2_FLAG_EXACT | K2_FLAG_EXACT_ANY)) return true;
    return o.exact_auto && o.variant < 0 && !(o.flags & (K2_FLAG_PRECISE | K2_FLAG_RECLO | K2_FLAG_STORE_ONLY | K2_FLAG_REC32));
}

// The options under which the exact-transform form is the only one that can run: 16-bit error images and per-frame cameras exist for nothing else.  0, or the
// first of three conditions that fails, in the order the entry points report them (k2_f16_check, k2_cams_check); the plan's 16-bit backstop asks the same.
enum { K2_EXONLY_OK = 0, K2_EXONLY_VARIANT = 1, K2_EXONLY_FLAGS = 2, K2_EXONLY_AUTO_OFF = 3 };
inline int k2_exact_only(int variant, int flags, bool exact_auto) {
    const int ex_bits = K2_FLAG_EXACT | K2_FLAG_EXACT_ANY;
    if (variant != -1) return K2_EXONLY_VARIANT;
    if (flags & ~(ex_bits | K2_FLAG_GENERAL_PATH)) return K2_EXONLY_FLAGS;  // the path knob selects no other form
    if (!exact_auto && !(flags & ex_bits)) return K2_EXONLY_AUTO_OFF;
    return K2_EXONLY_OK;
}

// The auto policy of the fp32 forms by size (measured on MI355X, profiles/r02_k2_variants.txt).  With the fused soft-inlier sums the kernel is VALU-limited:
// matrix-core form.  Error images only: store-limited, the VALU kernel with pixel tiles innermost has the best store stream (N = 256: 56.6 vs 58.9 us;
// N = 4096: equal).
// Round 3 (A/B inside bench.py on five boxes, profiles/r03_k2_ab_bench*.txt -- a plain-HIP harness, scripts/micro/k2_lab, ranks the forms differently from
// the bench's process and is NOT what this policy follows): big launches take the streaming form <32 hypotheses, 256 pixels> per one-wave workgroup (no LDS,
// no barrier, operands straight from the staged records, per-wave partial sums) in PLAIN pixel-minor block order: 842-870 us against 904-950 for round 2's
// <64,4> (0.73-0.75 of the HBM spec instead of 0.67-0.70); one frame of 256 hypotheses takes <64 hypotheses, 4 waves x 64 pixels>: 56.7-58.0 against 60.2-60.8 us.
// Late round 3: <64 hypotheses, 256 pixels> per one-wave workgroup at >= 4 waves per SIMD (form 58) instead of <32, 256> (form 45): 1 % ahead in every A/B on
// six boxes (profiles/r03_k2_ab_58_45.txt: 861-867 against 872-875 us alternating on one box) and half the partial-sum rows (with sampled pixel positions, or
// a map width that is not a multiple of 64, the kernel keeps the positions of every chunk in vector registers: form 58's 128-register build would spill
// 108-116 bytes per lane there, form 45 needs no scratch)
// By size (A/B inside bench.py at 2 ... 16 frames of 256 hypotheses per launch, profiles/r03_k2_ab_mid.txt): up to 1 GB of error images form 42 (2 frames:
// 111.7 us against 115.1 for form 45 and 121.6 for 58), up to 4.4 GB form 45 (4 frames 220.5 against 224 / 232; 8 frames 424-427 us = 0.75 of the HBM spec
// against 443 / 460-465; 12 frames 644 = 638-644), above it form 58 (16 frames: 861-867 against 872-875)
constexpr double K2_BIG_BYTES = 1.0e9, K2_HUGE_BYTES = 4.4e9;
inline double k2_err_bytes(int N, int P) { return (double)N * (double)P * 4.0; }
// the exact forms' tile switch: maps up to this many cells keep the <64 hypotheses, 64 cells> tile (a 40 x 40 map is 7 tiles of 256 pixels: one image per call
// 116 -> 127 us with them), larger ones take <64, 256>, which leaves a quarter of the partial-sum rows
constexpr int K2_SMALL_MAP_CELLS = 16384;

// Error images only on a big launch: the streaming form WITH the sigmoid arithmetic is the faster kernel -- the arithmetic spaces a wave's stores (N = 4096:
// 860 us against 890-900 for any form without it; idling the wave instead, k2_flags bits 16-23, does not reproduce the effect: profiles/r04_k2_err_ab.txt).
// So the auto policy runs that kernel and drops its partial sums (1200 x N floats of scratch, 0.4 % of the stores; no reduction launch).  k2_flags bit 24
// switches the policy off (A/B).
inline bool k2_fuse_sums(const K2Opts& o, int N, int P, bool want_err, bool want_soft) {
    return !want_soft && want_err && o.variant < 0 && !(o.flags & K2_FLAG_ERR_UNFUSED) && k2_err_bytes(N, P) > K2_BIG_BYTES;
}

// ---- the k2_variant ids --------------------------------------------------------------------------------------------------------------------------------
// One list: the plan resolves an id to its kernel family and tile from it, k2_variant_known() answers from it, and the launch switch of dk::reproject()
// expands it into its cases (the tile numbers are the kernels' template arguments).
//   VA(id, PX, HT, SPOSE)         k_reproject, VALU forms: PX pixels per thread, HT hypotheses per workgroup; SPOSE: scalar-load poses (SGPR operands)
//                                 instead of LDS-staged ones.  10..13 = 1, 2, 4, 8 hypothesis rows per workgroup
//   HP(id, HT, CH)                k_reproject_hp, matrix-core forms <HT hypotheses, CH 64-pixel chunks per wave>
//   ST(id, NG, CH, WV, PW, MINW)  k_reproject_st, streaming small-tile forms <NG 16-hypothesis groups, CH chunks per wave, WV waves per workgroup>; PW: per-wave
//                                 partial sums, no barrier (else through LDS, one row per workgroup); MINW: waves per SIMD the build is held to
//   PS(id, NG)                    k_reproject_ps, persistent pipelined forms <NG groups, 4 waves per workgroup>; k2_flags bits 8..15 = workgroups per CU
// 58 = <4,4,1> at >= 4 waves per SIMD, 59 = <2,4,1> at >= 5.  80..83 name the two-piece-record builds when k2_flags bit 27 is set (K2_RECLO_IDS) and 84 .. 95
// the exact-transform builds when bit 28 / 29 is (K2_EXACT_IDS); without the flag they are the plain form 58.
#define K2_FP32_IDS(VA, HP, ST, PS)                                                                                                                         \
    VA(0, 4, 32, false) VA(1, 4, 32, true) VA(2, 4, 16, false) VA(3, 4, 64, false) VA(10, 4, 1, false) VA(11, 4, 2, false) VA(12, 4, 4, false)               \
    VA(13, 4, 8, false)                                                                                                                                     \
    HP(20, 64, 2) HP(21, 64, 4) HP(22, 128, 2) HP(23, 32, 2) HP(24, 64, 1) HP(25, 128, 4) HP(26, 32, 4) HP(27, 128, 1)                                         \
    ST(40, 1, 1, 4, false, 1) ST(41, 2, 1, 4, false, 1) ST(42, 4, 1, 4, false, 1) ST(43, 2, 2, 4, false, 1)                                                   \
    ST(44, 1, 4, 1, true, 1) ST(45, 2, 4, 1, true, 1) ST(46, 4, 4, 1, true, 1) ST(47, 1, 2, 1, true, 1) ST(48, 2, 2, 1, true, 1) ST(49, 4, 2, 1, true, 1)       \
    ST(50, 1, 1, 1, true, 1) ST(51, 2, 1, 1, true, 1) ST(52, 4, 1, 1, true, 1) ST(53, 2, 1, 4, true, 1) ST(54, 2, 2, 4, true, 1) ST(55, 4, 1, 4, true, 1)       \
    ST(56, 2, 4, 4, true, 1) ST(57, 4, 2, 4, true, 1) ST(58, 4, 4, 1, true, 4) ST(59, 2, 4, 1, true, 5)                                                       \
    PS(60, 1) PS(61, 2) PS(62, 4)                                                                                                                           \
    ST(65, 4, 4, 4, true, 4) ST(66, 4, 4, 2, true, 4) ST(67, 1, 4, 4, true, 1) ST(68, 2, 4, 4, false, 1) ST(69, 2, 4, 8, true, 1) ST(70, 2, 4, 4, true, 4)     \
    ST(71, 1, 4, 8, true, 1) ST(72, 2, 4, 16, true, 1) ST(73, 2, 8, 1, true, 1) ST(74, 1, 8, 1, true, 1) ST(75, 2, 6, 1, true, 1) ST(76, 2, 3, 1, true, 1)     \
    ST(77, 1, 6, 1, true, 1)                                                                                                                                \
    ST(80, 4, 4, 1, true, 4) ST(81, 4, 4, 1, true, 4) ST(82, 4, 4, 1, true, 4) ST(83, 4, 4, 1, true, 4) ST(84, 4, 4, 1, true, 4) ST(85, 4, 4, 1, true, 4)     \
    ST(89, 4, 4, 1, true, 4) ST(93, 4, 4, 1, true, 4) ST(94, 4, 4, 1, true, 4) ST(95, 4, 4, 1, true, 4)
// Records in two pieces (k2_flags bit 27): the one-wave streaming form with the fp16 correction instructions, LO(id, NG, CH, MINW) -- the register / occupancy
// trades of this form (A/B).  80: <64 hypotheses, 256 pixels>, 3 waves per SIMD (92 B of scratch); 81: the same at 2 waves per SIMD, no scratch: the fastest of
// the four (profiles/r05_k2_reclo_ab.txt) and what the flag alone runs; 82: <64, 128>, 4 waves per SIMD; 83: <32, 256>, 3 waves per SIMD
#define K2_RECLO_IDS(LO) LO(80, 4, 4, 3) LO(81, 4, 4, 2) LO(82, 4, 2, 4) LO(83, 2, 4, 3)
constexpr int K2_RECLO_DEFAULT_ID = 81;
// The exact-transform vector build (k2_flags bit 28 / 29), EX(id, NG, CH, MINW, EXF): its tile / occupancy trades.  EXF 1 = reciprocal + Newton + square root,
// 2 = the one-transcendental tail.  84: <64, 256>, 2 waves per SIMD (three spill: 1.7 ms, profiles/r06_k2_exact_ab.txt); 85: 84 with tail 2; 89: <32, 256>;
// 93: <64, 64>, one-wave workgroups, 168 registers: 3 waves per SIMD; 94: 93 with tail 2; 95: 94 at four waves per SIMD (tail 2 needs 128 registers there).
// (85 .. 88 with a scheduling fence per m and 90 .. 92, <64, 4 waves x 64> and <64, 2 x 128>, were measured and removed: profiles/r06_k2_exact_ab.txt,
// r06_k2_exact_tiles.txt.)
#define K2_EXACT_IDS(EX) EX(84, 4, 4, 2, 1) EX(85, 4, 4, 2, 2) EX(89, 2, 4, 2, 1) EX(93, 4, 1, 3, 1) EX(94, 4, 1, 3, 2) EX(95, 4, 1, 4, 2)
// ... and what the auto policy runs, AX(NG, CH, MINW): tail 2 (968-987 against 1 002-1 020 us at the bench shape, the same or smaller errors:
// profiles/r06_k2_rsq_ab.txt, r06_k2_rsq_parity.txt) on the tile for the map's size (K2_SMALL_MAP_CELLS); for one frame of 256 hypotheses the <64, 64> tile is
// 0.8 us faster by itself (62.6 against 63.4) but leaves four times the partial-sum rows: k_reduce_soft 27.6 against 8.9 us (profiles/r06_one_image_trace.txt).
// Both tiles exist with EXF 2 (float error images), 3 / 4 (binary16: 8-byte stores / rows traded between neighbouring lanes, 16-byte stores; "k2_f16_store")
// and 5 / 6 (bfloat16, the same two layouts); the any-map build (K2_FORM_EXACT_ANY) takes the same two tiles.
#define K2_EXACT_AUTO_TILES(AX) AX(4, 1, 3) AX(4, 4, 2)

enum { K2_FAM_NONE = 0, K2_FAM_VALU_SCALAR, K2_FAM_VALU, K2_FAM_HP, K2_FAM_ST, K2_FAM_PS, K2_FAM_RECLO, K2_FAM_EXACT_VEC, K2_FAM_EXACT_ANY, K2_FAM_PRECISE };

// a kernel as the launch selects it: the family, the id of the fp32 / two-piece families (the launch switch's case) and the tile
//   VALU: px = PX, ht = HT;  HP: ht = HT, ch = CH;  ST / RECLO / EXACT_*: ng, ch, wv, pw, minw (exf: EXACT_VEC only);  PS: ng, wv = 4;  PRECISE: ht = 16 | 32
struct K2Kernel {
    int family = K2_FAM_NONE, id = -1;
    int px = 0, ht = 0, ng = 0, ch = 0, wv = 0, pw = 0, minw = 0, exf = 0;
};
inline K2Kernel k2_fp32_kernel(int id) {
    K2Kernel k;
    switch (id) {
#define K2_VA_(ID, PX, HT, SP) case ID: k.family = K2_FAM_VALU; k.id = ID; k.px = PX; k.ht = HT; break;
#define K2_HP_(ID, HT, CH) case ID: k.family = K2_FAM_HP; k.id = ID; k.ht = HT; k.ch = CH; break;
#define K2_ST_(ID, NG, CH, WV, PW, MW) case ID: k.family = K2_FAM_ST; k.id = ID; k.ng = NG; k.ch = CH; k.wv = WV; k.pw = PW; k.minw = MW; break;
#define K2_PS_(ID, NG) case ID: k.family = K2_FAM_PS; k.id = ID; k.ng = NG; k.wv = 4; break;
        K2_FP32_IDS(K2_VA_, K2_HP_, K2_ST_, K2_PS_)
#undef K2_VA_
#undef K2_HP_
#undef K2_ST_
#undef K2_PS_
        default: break;
    }
    return k;
}
inline K2Kernel k2_reclo_kernel(int id) {
    K2Kernel k;
    switch (id) {
#define K2_LO_(ID, NG, CH, MW) case ID: k.family = K2_FAM_RECLO; k.id = ID; k.ng = NG; k.ch = CH; k.wv = 1; k.pw = 1; k.minw = MW; break;
        K2_RECLO_IDS(K2_LO_)
#undef K2_LO_
        default: break;
    }
    return k;
}
inline K2Kernel k2_exact_kernel(int id) {
    K2Kernel k;
    switch (id) {
#define K2_EX_(ID, NG, CH, MW, F) case ID: k.family = K2_FAM_EXACT_VEC; k.id = ID; k.ng = NG; k.ch = CH; k.wv = 1; k.pw = 1; k.minw = MW; k.exf = F; break;
        K2_EXACT_IDS(K2_EX_)
#undef K2_EX_
        default: break;
    }
    return k;
}
// -1 (auto) or an id the launch has a kernel for
inline bool k2_variant_known(int v) { return v == -1 || k2_fp32_kernel(v).family != K2_FAM_NONE; }

// the largest count of partial-sum rows over all forms: one row per 64-pixel wave chunk, and the per-wave-sum forms with several waves per workgroup write
// PT * WAVES rows (their idle waves of the last workgroup write zero rows): up to WAVES - 1 <= 15 rows beyond ceil(P / 64).  soft_part holds this many rows
// of N floats (tests/test_k2_plan_cpu.py: no plan writes more)
inline int reproject_num_pixel_tiles(int P) { return (P + 63) / 64 + 15; }
inline int k2_ceil_div(int a, int b) { return (a + b - 1) / b; }
// the rows of soft_part a kernel writes on a map of P cells (soft: whether it writes sums at all -- only the any-map build's tail row depends on it)
inline int k2_tiles(const K2Kernel& k, int P, bool soft) {
    switch (k.family) {
        case K2_FAM_VALU_SCALAR: return k2_ceil_div(P, K2_WG);
        case K2_FAM_VALU: return k2_ceil_div(P, K2_WG * k.px);
        case K2_FAM_HP: return k2_ceil_div(P, K2_WG * k.ch);
        case K2_FAM_PS: return k2_ceil_div(P, 64);
        case K2_FAM_PRECISE: return 2 * k2_ceil_div(P, K2_WG * 4);  // a (high, low) pair of partial rows per pixel tile
        case K2_FAM_ST: case K2_FAM_RECLO: case K2_FAM_EXACT_VEC: case K2_FAM_EXACT_ANY: {
            const int PT = k2_ceil_div(P, k.wv * k.ch * 64);
            const int rows = k.pw ? PT * k.wv : PT;
            // any-map build: the tail launch for the last 1-3 cells of a map with P % 4 != 0 adds one row
            return rows + ((k.family == K2_FAM_EXACT_ANY && (P & 3) != 0 && soft) ? 1 : 0);
        }
        default: return 0;
    }
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------------------------
// everything the decision depends on.  The frame is the one the launch READS (its map, its buffers, its focal lengths)
struct K2PlanIn {
    K2Opts o;
    int N = 0, Nf = 0, frames = 1;  // Nf: hypotheses per frame of a frame batch (hypothesis h scores frame h / Nf), 0 = one frame
    int P = 0, W = 0;
    bool uv = false;                                        // sampled pixel positions given (else the implicit grid u = x, v = y)
    bool xyz_al16 = true, uv_al16 = true, err_al16 = true;  // the buffer sits on a 16-byte address (a NULL uv / err does)
    bool focal_ok = true;                                   // the focal lengths admit the split records (pose_split_available)
    bool poses = true;                                      // the cv poses exist (absent only in dsac_score_sampled: nothing to split)
    bool want_err = false, want_soft = false;               // what the CALLER wants; fuse_sums below may add the sums
    int err_elem = K2_ELEM_F32;
};
constexpr int K2_STATUS_OK = 0, K2_STATUS_INVALID = 1, K2_STATUS_NOT_SUPPORTED = 801;  // hipSuccess, hipErrorInvalidValue, hipErrorNotSupported
struct K2Plan {
    int status = K2_STATUS_OK;  // a refusal: nothing may be enqueued, every other field is as constructed
    int form = K2_FORM_NONE, why = 0;  // "k2_form_last" / "k2_form_why_last"; form NONE with status OK: an empty call (N or P 0, no output), nothing to launch
    K2Kernel k;
    bool need_split = false, need_lo = false;  // the records the kernel reads (pose_prep_split / pose_prep_lo)
    bool fuse_sums = false;     // error images only, but the kernel that also writes sums runs (k2_fuse_sums): soft_part is needed, its rows are dropped
    int kflags = 0;             // k2_flags as the kernel gets them; bit 5: plain pixel-minor block order instead of the XCD-aware one
    bool pixel_minor = true;    // block order of the VALU / matrix-core forms
    int Nf = 0;                 // as the kernels take it: one frame = N rounded up to 128 (every tile maps to frame 0)
    int tiles = 0;              // rows of soft_part the launch writes
    int hyp_walk = 1;           // consecutive hypothesis tiles of one frame a workgroup scores on its pixel tile (1, 2 or 4): the grid has that many times fewer workgroups
};

// ---- the hypothesis walk ---------------------------------------------------------------------------------------------------------------------------------
// The exact vector builds with a full-tile path (k_reproject_st: tail 2 or a 16-bit store, per-wave sums, at most 3 waves per SIMD, the implicit grid with
// W % 64 == 0) can score 2 or 4 consecutive hypothesis tiles of one frame per workgroup: the pixel tile's coordinates are loaded and split once per walk.
// Every (hypothesis, cell) is computed and stored exactly as with a walk of 1.
//   legal: no walk straddles the end of N or a frame -- N, and Nf of a frame batch, are multiples of the walk's hypotheses; else the next smaller length
//   "k2_hyp_walk" 1 / 2 / 4: that length where the kernel has the walk and it is legal
//   auto (0): only the regime of the <64, 256> tile at two waves per SIMD on more than K2_BIG_BYTES of error images (float-sized, whichever outputs are asked
//   for), and only while the launch is still K2_WALK_MIN_GENERATIONS fills of the chip's K2_WAVE_SLOTS wave slots: a walk of 4 on one frame of 256
//   hypotheses would be 0.6 fills of four-times-longer waves instead of 2.3 (measured: 88 against 61 us).  There the length is K2_WALK_AUTO, the fastest measured
//   at the bench shape, 16 x 256 x 640x480: K2 896 us at 4 and 900 at 2 against 920 at 1 (medians, profiles/k2_walk_path_ab.txt); bench.py's step 990.5-994.2 us
//   against the parent's 1 019.9-1 022.5, nine alternating runs each (profiles/k2_walk_bench_ab.txt)
constexpr int K2_WALK_AUTO = 4;
constexpr int K2_WAVE_SLOTS = 256 * 4 * 2;  // MI355X: 256 CUs x 4 SIMDs x the two waves per SIMD of the <64, 256> build
constexpr int K2_WALK_MIN_GENERATIONS = 8;  // the last, partly filled generation is then at most an eighth of the launch
inline bool k2_has_walk(const K2PlanIn& in, const K2Kernel& k) {
    return k.family == K2_FAM_EXACT_VEC && k.exf >= 2 && k.pw && k.wv == 1 && k.minw <= 3 && !in.uv && (in.W & 63) == 0;
}
inline bool k2_walk_legal(const K2PlanIn& in, const K2Kernel& k, int walk) {
    const int hyps = 16 * k.ng * walk;
    return in.N % hyps == 0 && (in.frames <= 1 || in.Nf <= 0 || in.Nf % hyps == 0);
}
// the hypothesis dimension of the streaming builds' grid: walks of `walk` tiles of 16 ng hypotheses (launch_reproject_st multiplies by the pixel tiles)
inline int k2_walks(int N, int ng, int walk) { return k2_ceil_div(k2_ceil_div(N, 16 * ng), walk); }
inline int k2_hyp_walk(const K2PlanIn& in, const K2Kernel& k) {
    if (!k2_has_walk(in, k)) return 1;
    int walk = in.o.hyp_walk;
    if (walk <= 0) {
        walk = K2_WALK_AUTO;
        if (!(k.ch == 4 && k.minw == 2 && k2_err_bytes(in.N, in.P) > K2_BIG_BYTES)) walk = 1;
        const long long wgs = (long long)k2_ceil_div(in.N, 16 * k.ng) * k2_ceil_div(in.P, 64 * k.ch);
        while (walk > 1 && wgs / walk < (long long)K2_WALK_MIN_GENERATIONS * K2_WAVE_SLOTS) walk >>= 1;
    }
    while (walk > 1 && !k2_walk_legal(in, k, walk)) walk >>= 1;
    return walk;
}

inline K2Plan k2_plan(const K2PlanIn& in) {
    K2Plan p;
    const K2Opts& o = in.o;
    const bool fuse = k2_fuse_sums(o, in.N, in.P, in.want_err, in.want_soft);
    const bool err = in.want_err, soft = in.want_soft || fuse;
    if (in.N <= 0 || in.P <= 0 || (!err && !soft)) return p;
    auto refuse = [](int status) { K2Plan r; r.status = status; return r; };
    if (in.Nf <= 0 || in.frames <= 1) p.Nf = ((in.N + 127) / 128) * 128;
    else if (in.Nf % K2_NF_MULTIPLE != 0) return refuse(K2_STATUS_INVALID);
    else p.Nf = in.Nf;
    p.fuse_sums = fuse;
    const int variant = o.variant;  // negative: the auto policy (-1; an id below it can only come from DSAC_K2_VARIANT and is held to what it has always run)
    // the 16-byte vector builds: H*W % 4 == 0 and every buffer aligned
    const bool vec = in.P % 4 == 0 && in.err_al16 && in.xyz_al16 && in.uv_al16;
    // the streaming / persistent forms (variant >= 40) know two block orders: XCD-aware pixel-minor (k2_order 1) and plain pixel-minor (k2_order 0 or bit 5)
    p.kflags = o.flags | ((variant >= 40 && !o.pixel_minor) ? 32 : 0);
    p.pixel_minor = o.pixel_minor;
    const bool split_ok = in.poses && k2_wants_exact(o) && in.focal_ok;  // the split records can be had and are wanted
    const K2Kernel exk = k2_exact_kernel(variant), lok = k2_reclo_kernel(variant);
    const bool ex_variant = exk.family != K2_FAM_NONE;
    // the reasons the exact form does not run
    int why = 0;
    if (!(o.flags & (K2_FLAG_EXACT | K2_FLAG_EXACT_ANY))) {
        if (variant >= 0 || (o.flags & (K2_FLAG_PRECISE | K2_FLAG_RECLO | K2_FLAG_STORE_ONLY | K2_FLAG_REC32))) why |= K2_WHY_FORCED;
        else if (!o.exact_auto) why |= K2_WHY_AUTO_OFF;
    } else if (variant >= 0 && !ex_variant) why |= K2_WHY_FORCED;
    if (!in.focal_ok) why |= K2_WHY_FOCAL;
    if (!in.poses) why |= K2_WHY_NO_POSES;
    // 16-bit error images: the auto policy's exact vector build and nothing else -- the entry points have refused every other request by name (k2_f16_check);
    // a launch that gets here all the same is an error, never another form and never a float store into a half buffer
    if (in.err_elem != K2_ELEM_F32 && !(err && vec && in.P % 8 == 0 && split_ok && k2_exact_only(variant, o.flags, o.exact_auto) == K2_EXONLY_OK))
        return refuse(K2_STATUS_NOT_SUPPORTED);
    // An arithmetic form that was ASKED for (k2_flags bits 25 / 27 / 28) and cannot run on this map -- its kernels read 16-byte vectors: H*W % 4, aligned buffers
    // and, on the implicit grid, four cells of a lane in one row; the exact form also needs a focal length <= 2^10 -- is an error, not a silent fp32 launch
    // (a parity run must not measure the fast form unknowingly).  The auto policy's exact form simply falls back.
    const bool prec_map = vec && (in.uv || in.W % 4 == 0);
    if (in.poses && (((o.flags & K2_FLAG_PRECISE) && !prec_map) || ((o.flags & K2_FLAG_RECLO) && !vec) || ((o.flags & K2_FLAG_EXACT) && !(vec && split_ok)) ||
                     ((o.flags & K2_FLAG_EXACT_ANY) && !(split_ok && (variant < 0 || (ex_variant && vec))))))
        return refuse(K2_STATUS_NOT_SUPPORTED);
    // bit 29 (EXACT, any map) is what a parity run sets: besides the focal length only what would make it another form rules it out -- a k2_variant that names
    // another form (the tile / tail trades 84 .. 95 exist in the vector build only), or a call without the cv poses the records are split from
    if ((o.flags & K2_FLAG_EXACT_ANY) && !in.poses) return refuse(K2_STATUS_NOT_SUPPORTED);
    const bool small_map = in.P <= K2_SMALL_MAP_CELLS;
    if ((o.flags & K2_FLAG_PRECISE) && in.poses && prec_map) {
        // the precise form works from the cv poses themselves; hypothesis tile by size as the VALU forms: 32 for big launches, 16 for a single small frame
        p.form = K2_FORM_PRECISE;
        p.k.family = K2_FAM_PRECISE;
        p.k.ht = (double)in.N * (double)in.P > 2.0e8 ? 32 : 16;
    } else if ((o.flags & K2_FLAG_RECLO) && in.poses && vec && (variant < 0 || lok.family != K2_FAM_NONE)) {
        p.form = K2_FORM_RECLO;
        p.k = variant < 0 ? k2_reclo_kernel(K2_RECLO_DEFAULT_ID) : lok;
        p.need_lo = true;
        p.kflags |= 32;
    } else if (k2_wants_exact(o) && split_ok && (vec ? (variant < 0 || ex_variant) : variant < 0)) {
        // Maps the vector build cannot read (H*W % 4, a buffer off the 16-byte grid) take the ANY build of the same kernel on the auto policy's tile for their
        // size: the same arithmetic per cell, the same tile for the same P, so the two builds agree bit for bit on the same cells (but for groups that hold a
        // hypothesis with clamped records, which only the ANY build sends through the fp32 transform: grp_far)
        p.form = vec ? K2_FORM_EXACT_VEC : K2_FORM_EXACT_ANY;
        if (variant >= 0) p.k = exk;
        else if (vec && variant != -1) p.k = k2_exact_kernel(84);  // the vector build's first trade, not the policy's tile: what such an id has always run
        else {
            p.k = k2_exact_kernel(small_map ? 94 : 85);  // the auto policy's two tiles with tail 2, K2_EXACT_AUTO_TILES
            p.k.id = -1;
            if (in.err_elem == K2_ELEM_F16) p.k.exf = o.f16_store == 0 ? 3 : 4;
            if (in.err_elem == K2_ELEM_BF16) p.k.exf = o.f16_store == 0 ? 5 : 6;
        }
        p.k.family = vec ? K2_FAM_EXACT_VEC : K2_FAM_EXACT_ANY;
        p.need_split = true;
        p.kflags |= 32;
    } else if (!vec) {
        p.form = K2_FORM_FP32_VALU;
        p.k.family = K2_FAM_VALU_SCALAR;  // one pixel per thread, 32 hypotheses per workgroup, whatever the id
    } else {
        int id = variant;
        if (variant < 0) {
            const double bytes = k2_err_bytes(in.N, in.P);
            const bool big = bytes > K2_BIG_BYTES;
            const bool grid64 = !in.uv && (in.W & 63) == 0;
            id = soft ? (big ? ((grid64 && bytes > K2_HUGE_BYTES) ? 58 : 45) : 42) : 0;
            if (soft && big) p.kflags |= 32;
            p.pixel_minor = true;  // the auto policy's forms were all measured with pixel tiles innermost
        }
        p.k = k2_fp32_kernel(id);
        if (p.k.family == K2_FAM_NONE) return refuse(K2_STATUS_INVALID);                            // unknown id
        if (p.k.family == K2_FAM_PS && in.N % 4 != 0 && soft) return refuse(K2_STATUS_INVALID);      // its partial sums leave as 16-byte stores
        p.form = (variant < 0 ? !soft : variant <= 13) ? K2_FORM_FP32_VALU : K2_FORM_FP32_MFMA;
    }
    p.why = (p.form == K2_FORM_EXACT_VEC || p.form == K2_FORM_EXACT_ANY) ? 0 : why;
    p.tiles = k2_tiles(p.k, in.P, soft);
    p.hyp_walk = k2_hyp_walk(in, p.k);
    return p;
}

}  // namespace dk
