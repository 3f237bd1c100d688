// k_forward.hip -- forward kernels of the gfx950 DSAC engine.
//
//   pose_prep   : fp64 Rodrigues of the N cv poses -> 48-byte float records (intrinsics folded in)
//   k_reproject : K2, the N x P reprojection / error-image / soft-inlier kernel (HBM-write bound)
//   reduce_soft : deterministic second stage of the soft-inlier sums
//   softmax     : K3, softmax + entropy + soft-argmax pose (fp64, one workgroup)
//
// K2 replaces the N getDiffMap calls of the reference (core/cnn_softam.h:1067-1069, getDiffMap :319-362).
// Data layout in HBM:  xyz  P x 3 f32 (AoS, 12 B/pixel, read once per hypothesis tile, L2-resident),
//                      err  N x P f32 hypothesis-major (written once, streaming, non-temporal),
//                      staged poses N x 12 f32.
// Work decomposition: a workgroup of 256 lanes owns a tile of 1024 consecutive pixels (4 per lane, so that
// every global access is a 16-byte dwordx4 and one wave store covers 1 KiB of one error-image row) and a
// tile of HT hypotheses whose 3x4 records are staged in LDS and broadcast to all lanes.  The block index is
// decoded XCD-aware: blocks that share a pixel tile run on the same XCD (block b -> XCD b % 8) back to
// back, so the xyz tile is fetched from HBM once and re-read from that XCD's L2.
#include "kernels.h"
#include <hip/hip_ext.h>
#include "dmath.h"

namespace dk {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// --------------------------------------------------------------------------------------------------
// Per-frame cameras (FrameDev::cams) in the record kernels: hypothesis h of a batch folds the focal lengths of its own frame h / Nf (Nf <= 0: one frame, row 0),
// and the split records that frame's own exponent -- what the single-frame call under that camera folds, bit for bit.
DM_INLINE void pose_focal(const float4* __restrict__ cams, int h, int Nf, float& fx, float& fy) {
    if (!cams) return;
    const float4 k = cams[Nf > 0 ? h / Nf : 0];
    fx = k.x; fy = k.y;
}
DM_INLINE int split_exponent_of(float fx, float fy) {  // pose_split_exponent's loop; a power of two up to 2^31 is exact as a float, as ldexp's double is
    int e = 0;
    while (e < 31 && (float)(1u << e) < fmaxf(fx, fy)) e++;
    return e;
}
__global__ __launch_bounds__(256) void k_pose_prep(int N, const double* __restrict__ poses, float fx, float fy, float* __restrict__ staged,
                                                   const float4* __restrict__ cams, int Nf) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= N) return;
    pose_focal(cams, h, Nf, fx, fy);
    double r[3] = {poses[6 * h], poses[6 * h + 1], poses[6 * h + 2]};
    double R[9];
    dm::rodrigues_v2m<false>(r, R, nullptr);
    const double t0 = poses[6 * h + 3], t1 = poses[6 * h + 4], t2 = poses[6 * h + 5];
    float* o = staged + (size_t)h * POSE_STRIDE;
    const double dfx = fx, dfy = fy;
    o[0] = (float)(dfx * R[0]); o[1] = (float)(dfx * R[1]); o[2] = (float)(dfx * R[2]); o[3] = (float)(dfx * t0);
    o[4] = (float)(dfy * R[3]); o[5] = (float)(dfy * R[4]); o[6] = (float)(dfy * R[5]); o[7] = (float)(dfy * t1);
    o[8] = (float)R[6]; o[9] = (float)R[7]; o[10] = (float)R[8]; o[11] = (float)t2;
}

// What the float records leave behind: lo = (float)(A - (double)(float)A) for the twelve entries of k_pose_prep's record (the same fp64 arithmetic, so
// the pair is consistent with the records K1 stages itself).  k2_flags bit 27.
__global__ __launch_bounds__(256) void k_pose_prep_lo(int N, const double* __restrict__ poses, float fx, float fy, float* __restrict__ staged_lo,
                                                      const float4* __restrict__ cams, int Nf) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= N) return;
    pose_focal(cams, h, Nf, fx, fy);
    double r[3] = {poses[6 * h], poses[6 * h + 1], poses[6 * h + 2]};
    double R[9];
    dm::rodrigues_v2m<false>(r, R, nullptr);
    const double dfx = fx, dfy = fy;
    const double A[12] = {dfx * R[0], dfx * R[1], dfx * R[2], dfx * poses[6 * h + 3], dfy * R[3], dfy * R[4], dfy * R[5], dfy * poses[6 * h + 4],
                          R[6], R[7], R[8], poses[6 * h + 5]};
    float* o = staged_lo + (size_t)h * POSE_STRIDE;
#pragma unroll
    for (int k = 0; k < 12; k++) o[k] = (float)(A[k] - (double)(float)A[k]);
}

hipError_t pose_prep_lo(hipStream_t st, int N, const double* poses, const FrameDev& F, float* staged_lo, int Nf) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pose_prep_lo, dim3((N + 255) / 256), dim3(256), 0, st, N, poses, F.fx, F.fy, staged_lo, F.cams, Nf);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------
// Round 6: the pose records as fp16 PIECES on fixed binary grids, for the exact-transform form of K2 (k2_flags bit 28; k_reproject_st<.., EX>).
// The reference projects in double (core/cnn_softam.h:319-362).  E = R.X + t is evaluated here without any rounding that matters by writing both factors as
// sums of short fixed-point pieces whose products are exact in fp32 and by sorting the products into TWO matrix-core accumulations:
//   * the HIGH group -- every product that is a multiple of 2^(E-5) -- is summed EXACTLY by one v_mfma_f32_16x16x16_f16 per row (all addends on one grid,
//     |sum| < 2^23 grid units):  aA XA + aT XM + aBT XT + tA + tA2;
//   * the CROSS group -- what is left, |sum| of a few millimetres -- by one v_mfma_f32_16x16x32_f16 per row, scaled by 2^14 so that every half is a
//     NORMAL number (the matrix core flushes subnormal halves):  aC XA + aA' XM + aB' XT + aA XL1 + aA XL2 + aB XA' + aB XM + aB XL1 + tC + tD;
//   * E = D_hi + 2^-14 D_cross: one fused multiply-add, the single rounding to float of the camera-frame point.
// Why the split is where it is: the fp16 matrix core aligns the products of one instruction to the LARGEST of them, keeps ~24 bits and TRUNCATES the rest
// (profiles/r06_mfma_f16_numerics.txt: 2^14 + 0.75 ulp -> 2^14; 2^14 - 2^14 + 2^-12 -> 0).  The first design of this form put every product but aA XA + tA
// into the cross group (largest addends ~2^5 mm): the truncation of its small addends, whose signs follow the hypothesis, shifted a hypothesis' points by
// ~1e-6 mm systematically -- enough to move the softmax weight of two tied hypotheses by 1.5-2.2e-4 (stated 1e-4; profiles/r06_k2_diag.txt).  With the three
// largest remainders moved into the exact group the cross sum stays below ~4 mm and what its window drops is below 2^-22 mm.
// Pieces (E = 0 for the z row, `ex` = ceil(log2 f) <= 10 for the focal-length-folded x / y rows; n x 2^g = an integer |n| <= 2047 times the grid 2^g):
//   a = aA + aB + aC     aA: 2^(E-10)   aB: 2^(E-21)   aC: 2^(E-32)        aA = aT + aA', aT: 2^(E-5)        aB = aBT + aB', aBT: 2^(E-15)
//   X = XA + XM + XL1 + XL2    XA: 32 rint(X / 32) = XT + XA', XT: 1024 rint(X / 1024)    XM: rint(X - XA)    XL1: 2^-12 rint(.)    XL2: the rest (< 2^-13)
//   t = tA + tA2 + tC + tD     tA: 2^(E+6)   tA2: 2^(E-5)   tC: 2^(E-16)   tD: 2^(E-27)
// What this kernel writes is the A-operand image in the matrix core's own lane layout: for hypothesis h, row r in (x, y, z), quarter q (= coordinate X, Y, Z,
// or the translation for q = 3): eight halves for the K = 32 instruction (k = 8q .. 8q + 7) and four for the K = 16 one (k = 4q .. 4q + 3), whose B operand
// is the FIRST HALF of the other's:
//   B[q < 3]     = (XA 2^-5,   XM 2^3,    XT 2^-4,   XL1 2^10,  XL2 2^10,  XA',     XM,       XL1   )
//   hi[q < 3]    = (aA 2^5,    aT 2^-3,   aBT 2^4,   0)
//   cross[q < 3] = (aC 2^19,   aA' 2^11,  aB' 2^18,  aA 2^4,    aA 2^4,    aB 2^14, aB 2^14,  aB 2^14)
//   B[q = 3]     = (2^10, 2^3, 2^11, 0, 0, 0, 1, 0) -- the pieces of the constant 2^15 + 1 run through the same code as a coordinate
//   hi[q = 3]    = (0, tA2 2^-3, tA 2^-11, 0)          cross[q = 3] = (0, tC 2^11, 0, 0, 0, 0, tD 2^14, 0)
// The x and y rows carry the minus sign of hp_chunk's (-xc, -yc, zc).  Valid for focal lengths up to 2^10 px, |t| < 2^16 mm, |X| < 2^16 mm (the kernel
// sends chunks with larger coordinates down the fp32 path); pieces are clamped to +-2047 grid units, so out-of-range input degrades, it does not overflow.
// --------------------------------------------------------------------------------------------------
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
constexpr int SPLIT_CROSS_BYTES = 12 * 16, SPLIT_HI_BYTES = 12 * 8;  // per hypothesis: 3 rows x 4 quarters
constexpr int SPLIT_MAX_EX = 10;  // pose_split_exponent above this: no exact form (api.hip falls back to the fp32 records)
DM_INLINE double split_piece(double& rem, int grid_exp) {  // the multiple of 2^grid_exp nearest to rem (at most 2047 units), which is taken out of rem
    double n = rint(ldexp(rem, -grid_exp));
    n = fmin(fmax(n, -2047.0), 2047.0);
    const double p = ldexp(n, grid_exp);
    rem -= p;
    return p;
}
DM_INLINE _Float16 hf(double v, int e) { return (_Float16)(float)ldexp(v, e); }
// does the split of one record row (three rotation entries and the translation, focal length folded in) clamp a piece or meet a non-finite entry?  Such a
// hypothesis is outside the exact form's range (|t_z| >= 2047.5 x 2^6 mm, |f t_x| >= 2047.5 x 2^(E+6)): k_pose_prep_split marks it in the one half of its record
// that multiplies a zero of the B operand, the any-map build of K2 sends its group down the fp32 transform, dsac_k2_range_census counts it
DM_INLINE bool split_piece_bad(double& rem, int grid_exp) {  // split_piece, returning whether the piece had to be clamped (or is not a number)
    const double n = rint(ldexp(rem, -grid_exp));
    rem -= ldexp(fmin(fmax(n, -2047.0), 2047.0), grid_exp);
    return !(fabs(n) <= 2047.0);
}
DM_INLINE bool split_row_bad(const double (&a)[4], int E) {
    bool bad = false;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        double rem = a[q];
        bad |= !(fabs(rem) < 1.0e300);
        bad |= split_piece_bad(rem, E - 10); bad |= split_piece_bad(rem, E - 21); bad |= split_piece_bad(rem, E - 32);
    }
    double rem = a[3];
    bad |= !(fabs(rem) < 1.0e300);
    bad |= split_piece_bad(rem, E + 6); bad |= split_piece_bad(rem, E - 5); bad |= split_piece_bad(rem, E - 16); bad |= split_piece_bad(rem, E - 27);
    return bad;
}
__global__ __launch_bounds__(256) void k_pose_prep_split(int N, const double* __restrict__ poses, float fx, float fy, int ex, h8* __restrict__ cross, h4* __restrict__ hi,
                                                         const float4* __restrict__ cams, int Nf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // one thread per (hypothesis, row)
    const int h = i / 3, r = i - 3 * h;
    if (h >= N) return;
    if (cams) {
        pose_focal(cams, h, Nf, fx, fy);
        ex = split_exponent_of(fx, fy);
    }
    double rv[3] = {poses[6 * h], poses[6 * h + 1], poses[6 * h + 2]};
    double R[9];
    dm::rodrigues_v2m<false>(rv, R, nullptr);
    const double f = r == 0 ? -(double)fx : r == 1 ? -(double)fy : 1.0;
    const int E = r < 2 ? ex : 0;
    const double a[4] = {f * R[3 * r], f * R[3 * r + 1], f * R[3 * r + 2], f * poses[6 * h + 3 + r]};
    h8* oc = cross + ((size_t)h * 3 + r) * 4;
    h4* oh = hi + ((size_t)h * 3 + r) * 4;
    const _Float16 z = (_Float16)0.f;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        double rem = a[q];
        const double aA = split_piece(rem, E - 10), aB = split_piece(rem, E - 21), aC = split_piece(rem, E - 32);
        double t1 = aA, t2 = aB;
        const double aT = split_piece(t1, E - 5), aBT = split_piece(t2, E - 15);  // t1 = aA' (|aA'| <= 2^(E-6)), t2 = aB' (<= 2^(E-16))
        oh[q] = h4{hf(aA, 5), hf(aT, -3), hf(aBT, 4), z};
        oc[q] = h8{hf(aC, 19), hf(t1, 11), hf(t2, 18), hf(aA, 4), hf(aA, 4), hf(aB, 14), hf(aB, 14), hf(aB, 14)};
    }
    double rem = a[3];
    const double tA = split_piece(rem, E + 6), tA2 = split_piece(rem, E - 5), tC = split_piece(rem, E - 16), tD = split_piece(rem, E - 27);
    // against B[q = 3] = the pieces of SPLIT_T_COORD = (2^10, 2^3, 2^11, 0, 0, 0, 1, 0)
    // the fourth half meets the 0 of B[q = 3]: the product is an exact zero whatever it holds, so it carries the out-of-range mark (1 or 0) for free
    oh[3] = h4{z, hf(tA2, -3), hf(tA, -11), split_row_bad(a, E) ? (_Float16)1.f : z};
    oc[3] = h8{z, hf(tC, 11), z, z, z, z, hf(tD, 14), z};
}

size_t pose_split_bytes(int N) { return (size_t)N * (SPLIT_CROSS_BYTES + SPLIT_HI_BYTES); }
bool pose_split_available(const FrameDev& F) { return pose_split_exponent(F) <= SPLIT_MAX_EX; }
// ceil(log2(max focal length)), at least 0; > SPLIT_MAX_EX = 10: the exact form is not available.  With per-frame cameras: the largest over the frames (what
// decides whether the form is available); the records of frame f fold that frame's own exponent (k_pose_prep_split)
int pose_split_exponent(const FrameDev& F) {
    float fm = fmaxf(F.fx, F.fy);
    if (F.cams_h)
        for (int f = 0; f < (F.frames > 1 ? F.frames : 1); f++) fm = fmaxf(fm, fmaxf(F.cams_h[4 * f], F.cams_h[4 * f + 1]));
    int e = 0;
    while (ldexp(1.0, e) < (double)fm) e++;
    return e;
}
hipError_t pose_prep_split(hipStream_t st, int N, const double* poses, const FrameDev& F, void* split, int Nf) {
    if (N <= 0) return hipSuccess;
    h8* cross = reinterpret_cast<h8*>(split);
    h4* hi = reinterpret_cast<h4*>(reinterpret_cast<char*>(split) + (size_t)N * SPLIT_CROSS_BYTES);
    hipLaunchKernelGGL(k_pose_prep_split, dim3((3 * N + 255) / 256), dim3(256), 0, st, N, poses, F.fx, F.fy, pose_split_exponent(F), cross, hi, F.cams, Nf);
    return hipGetLastError();
}

hipError_t pose_prep(hipStream_t st, int N, const double* poses, const FrameDev& F, float* staged, int Nf) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pose_prep, dim3((N + 255) / 256), dim3(256), 0, st, N, poses, F.fx, F.fy, staged, F.cams, Nf);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------
// K2
// --------------------------------------------------------------------------------------------------
constexpr int K2_THREADS = 256;

DM_INLINE float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One residual.  r0/r1 carry the focal length, (pu, pv) are the pixel position minus the principal point.
DM_INLINE float residual(const f4 r0, const f4 r1, const f4 r2, float X, float Y, float Z, float pu, float pv, float clampv) {
    const float xc = fmaf(r0.x, X, fmaf(r0.y, Y, fmaf(r0.z, Z, r0.w)));
    const float yc = fmaf(r1.x, X, fmaf(r1.y, Y, fmaf(r1.z, Z, r1.w)));
    const float zc = fmaf(r2.x, X, fmaf(r2.y, Y, fmaf(r2.z, Z, r2.w)));
    // projectPoints: z = Z ? 1/Z : 1
    const float iz = (zc == 0.0f) ? 1.0f : __builtin_amdgcn_rcpf(zc);
    const float du = fmaf(-xc, iz, pu);
    const float dv = fmaf(-yc, iz, pv);
    const float d2 = fmaf(dv, dv, du * du);
    return fminf(__builtin_amdgcn_sqrtf(d2), clampv);
}

// sigmoid(beta * (tau - e)) = 1 / (1 + 2^(kA * e + kB))  with kA = beta*log2(e), kB = -beta*tau*log2(e)
DM_INLINE float soft_inlier(float e, float kA, float kB) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(fmaf(kA, e, kB)));
}

// Packed-fp32 forms: two pixels per VALU instruction (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32).  K2 is
// VALU-issue bound once the stores stream (rocprof: SQ_ACTIVE_INST_VALU ~ all SIMD cycles), and a packed op
// issues in the time of a scalar one, so the 9-FMA rigid transform and the residual arithmetic run at
// half the issue cost; only rcp / sqrt / exp2 (transcendental pipe) and min stay per pixel.
DM_INLINE f2 splat(float a) { return f2{a, a}; }
DM_INLINE f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

DM_INLINE f2 residual2(const f4 r0, const f4 r1, const f4 r2, f2 X, f2 Y, f2 Z, f2 pu, f2 pv, float clampv) {
    const f2 xc = pk_fma(splat(r0.x), X, pk_fma(splat(r0.y), Y, pk_fma(splat(r0.z), Z, splat(r0.w))));
    const f2 yc = pk_fma(splat(r1.x), X, pk_fma(splat(r1.y), Y, pk_fma(splat(r1.z), Z, splat(r1.w))));
    const f2 zc = pk_fma(splat(r2.x), X, pk_fma(splat(r2.y), Y, pk_fma(splat(r2.z), Z, splat(r2.w))));
    f2 iz;
    iz.x = (zc.x == 0.0f) ? 1.0f : __builtin_amdgcn_rcpf(zc.x);
    iz.y = (zc.y == 0.0f) ? 1.0f : __builtin_amdgcn_rcpf(zc.y);
    const f2 du = pk_fma(-xc, iz, pu);
    const f2 dv = pk_fma(-yc, iz, pv);
    const f2 d2 = pk_fma(dv, dv, du * du);
    f2 e;
    e.x = fminf(__builtin_amdgcn_sqrtf(d2.x), clampv);
    e.y = fminf(__builtin_amdgcn_sqrtf(d2.y), clampv);
    return e;
}

DM_INLINE f2 soft_inlier2(f2 e, float kA, float kB) {
    const f2 t = pk_fma(splat(kA), e, splat(kB));
    f2 ex;
    ex.x = __builtin_amdgcn_exp2f(t.x);
    ex.y = __builtin_amdgcn_exp2f(t.y);
    const f2 d = ex + splat(1.0f);
    f2 s;
    s.x = __builtin_amdgcn_rcpf(d.x);
    s.y = __builtin_amdgcn_rcpf(d.y);
    return s;
}

template <int PX, int HT, bool ERR, bool SOFT, bool UV, bool SPOSE>
__global__ __launch_bounds__(K2_THREADS) void k_reproject(const float* __restrict__ staged, const float* __restrict__ xyz,
                                                          const float* __restrict__ uv, float* __restrict__ err,
                                                          float* __restrict__ soft_part, int N, int P, int W, int PT, int NT, float cx,
                                                          float cy, float clampv, float kA, float kB, int kflags, int Nf, long long xyz_stride,
                                                          long long uv_stride) {
    // XCD-aware decode: the 8 blocks of one dispatch round-robin group cover 8 different pixel tiles, and
    // successive groups walk the hypothesis tiles of those same pixel tiles.
    const int b = blockIdx.x;
    const int q = b >> 3;
    // order: NT > 0 -> hypothesis tiles innermost (same pixel tile back to back);  NT < 0 -> pixel tiles
    // innermost (the resident blocks write a contiguous band of error-image rows), |NT| hypothesis tiles.
    int ht, pt;
    if (NT > 0) { ht = q % NT; pt = (q / NT) * 8 + (b & 7); }
    else { const int PTG = (PT + 7) >> 3; ht = q / PTG; pt = (q % PTG) * 8 + (b & 7); }
    if (pt >= PT) return;
    const int h0 = ht * HT;
    const int nh = min(HT, N - h0);
    const int tid = threadIdx.x;
    {   // frame batch: all hypotheses of this tile score the same frame (Nf is a multiple of HT)
        const int frame = h0 / Nf;
        xyz += (long long)frame * xyz_stride;
        if (UV) uv += (long long)frame * uv_stride;
    }

    __shared__ __attribute__((aligned(16))) float s_pose[HT * POSE_STRIDE];
    __shared__ float s_red[SOFT ? (K2_THREADS / 64) * HT : 1];
    if (!SPOSE) {
        for (int i = tid; i < nh * POSE_STRIDE; i += K2_THREADS) s_pose[i] = staged[(size_t)h0 * POSE_STRIDE + i];
    }

    const int p0 = (pt * K2_THREADS + tid) * PX;
    const bool valid = p0 < P;  // PX == 4 is only launched with P % 4 == 0
    float X[PX], Y[PX], Z[PX], pu[PX], pv[PX];
    if (PX == 4) {
        if (valid) {
            const f4* src = reinterpret_cast<const f4*>(xyz + (size_t)p0 * 3);
            const f4 a = src[0], bb = src[1], c = src[2];
            X[0] = a.x; Y[0] = a.y; Z[0] = a.z;
            X[1] = a.w; Y[1] = bb.x; Z[1] = bb.y;
            X[2] = bb.z; Y[2] = bb.w; Z[2] = c.x;
            X[3] = c.y; Y[3] = c.z; Z[3] = c.w;
            if (UV) {
                const f4* su = reinterpret_cast<const f4*>(uv + (size_t)p0 * 2);
                const f4 u0 = su[0], u1 = su[1];
                pu[0] = u0.x - cx; pv[0] = u0.y - cy; pu[1] = u0.z - cx; pv[1] = u0.w - cy;
                pu[2] = u1.x - cx; pv[2] = u1.y - cy; pu[3] = u1.z - cx; pv[3] = u1.w - cy;
            }
        } else {
#pragma unroll
            for (int k = 0; k < PX; k++) { X[k] = Y[k] = 0.f; Z[k] = 1.f; pu[k] = pv[k] = 0.f; }
        }
    } else {
        if (valid) {
            X[0] = xyz[(size_t)p0 * 3]; Y[0] = xyz[(size_t)p0 * 3 + 1]; Z[0] = xyz[(size_t)p0 * 3 + 2];
            if (UV) { pu[0] = uv[(size_t)p0 * 2] - cx; pv[0] = uv[(size_t)p0 * 2 + 1] - cy; }
        } else { X[0] = Y[0] = 0.f; Z[0] = 1.f; pu[0] = pv[0] = 0.f; }
    }
    if (!UV) {
#pragma unroll
        for (int k = 0; k < PX; k++) {
            const int p = p0 + k;
            const int y = p / W, x = p - y * W;
            pu[k] = (float)x - cx;
            pv[k] = (float)y - cy;
        }
    }
    if (!SPOSE) __syncthreads();

    float* erow = ERR ? err + (size_t)h0 * P + p0 : nullptr;
    const int wave = tid >> 6, lane = tid & 63;

#pragma unroll 4
    for (int h = 0; h < HT; h++) {
        if (h < nh) {
            f4 r0, r1, r2;
            if (SPOSE) {
                const f4* sp = reinterpret_cast<const f4*>(staged + (size_t)(h0 + h) * POSE_STRIDE);
                r0 = sp[0]; r1 = sp[1]; r2 = sp[2];
            } else {
                const f4* sp = reinterpret_cast<const f4*>(s_pose + h * POSE_STRIDE);
                r0 = sp[0]; r1 = sp[1]; r2 = sp[2];
            }
            float e[PX];
            if (PX % 2 == 0) {
#pragma unroll
                for (int k = 0; k < PX; k += 2) {
                    const f2 e2 = residual2(r0, r1, r2, f2{X[k], X[k + 1]}, f2{Y[k], Y[k + 1]}, f2{Z[k], Z[k + 1]}, f2{pu[k], pu[k + 1]},
                                            f2{pv[k], pv[k + 1]}, clampv);
                    e[k] = e2.x; e[k + 1] = e2.y;
                }
            } else {
#pragma unroll
                for (int k = 0; k < PX; k++) e[k] = residual(r0, r1, r2, X[k], Y[k], Z[k], pu[k], pv[k], clampv);
            }
            if (ERR && valid) {
                if (PX == 4) {
                    f4 o = {e[0], e[1], e[2], e[3]};
                    if (kflags & 1) *reinterpret_cast<f4*>(erow + (size_t)h * P) = o; else __builtin_nontemporal_store(o, reinterpret_cast<f4*>(erow + (size_t)h * P));
                } else {
                    __builtin_nontemporal_store(e[0], erow + (size_t)h * P);
                }
            }
            if (SOFT) {
                float s = 0.f;
                if (PX % 2 == 0) {
                    f2 s2 = splat(0.f);
#pragma unroll
                    for (int k = 0; k < PX; k += 2) s2 += soft_inlier2(f2{e[k], e[k + 1]}, kA, kB);
                    s = s2.x + s2.y;
                } else {
#pragma unroll
                    for (int k = 0; k < PX; k++) s += soft_inlier(e[k], kA, kB);
                }
                s = wave_sum(valid ? s : 0.f);
                if (lane == 0) s_red[wave * HT + h] = s;
            }
        }
    }

    if (SOFT) {
        __syncthreads();
        if (tid < nh) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < K2_THREADS / 64; w++) s += s_red[w * HT + tid];
            soft_part[(size_t)pt * N + h0 + tid] = s;
        }
    }
}

// --------------------------------------------------------------------------------------------------
// K2, matrix-core form.  The rigid transform of all pixels under all hypotheses is the product
// [3N x 4] (rows R_i | t_i of every pose) x [4 x P] (X, Y, Z, 1 of every pixel) -- a GEMM with K = 4, which is
// exactly one v_mfma_f32_16x16x4_f32 per 16 x 16 output tile (fp32 in, fp32 accumulate, bit-equal to an fmaf
// chain).  rocprof showed the all-VALU kernel issue-bound on the vector ALUs (SQ_ACTIVE_INST_VALU ~ every
// SIMD cycle) with HBM at ~63 %; the 9 FMAs per (hypothesis, pixel) move to the matrix pipe, which runs
// concurrently with the VALU.  (Round 1's operand layout -- rows (hypothesis, x/y/z/pad), one pair per lane -- is gone: the
// hypothesis-pair layout below needs 12 instead of 16 MFMAs per 1024 pairs and half the VALU work; see k_reproject_hp.)
// --------------------------------------------------------------------------------------------------
DM_INLINE float row16_sum(float v) {  // sum over the 16 lanes of a DPP row, result in every lane
    int x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xf, 0xf, true));  // row_half_mirror
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x140, 0xf, 0xf, true));  // row_mirror
    return v;
}

// --------------------------------------------------------------------------------------------------
// K2, matrix-core form with HYPOTHESIS-PAIR packed finishing (round 2).  Same GEMM, other operand roles: per group of 16 hypotheses
// three A operands hold their x-, y- and z-rows (A_x[i][k] = fx R0[k] | fx t0 of hypothesis i, ...), B is unchanged (X, Y, Z, 1 of the
// pixel columns).  D_x / D_y / D_z of one v_mfma_f32_16x16x4_f32 each then give lane (g, c) the SAME component of FOUR hypotheses
// (4g .. 4g+3) for pixel column c in four adjacent registers, so every finishing operation runs packed over a hypothesis pair
// (v_pk_fma_f32 / v_pk_mul_f32: du, dv, du^2 + dv^2, the sigmoid's affine map and 1 + 2^t), the pixel position is a broadcast operand,
// and there is no padding row: 12 MFMAs per 1024 (hypothesis, pixel) pairs instead of 16, ~5 plain VALU operations per pair instead of
// ~11 (the 4 transcendentals per pair -- rcp z, sqrt, exp2, rcp -- are what is left).  With m = 0..3 as before (column c -> pixel
// 4c + m) a lane ends up with 4 consecutive pixels of each of its 4 hypotheses: four dwordx4 stores, each wave store still 4 rows x 256 B.
// Arithmetic per pair is the VALU kernel's (fma(dv, dv, du*du)), the transform is the exact fp32 MFMA.
// --------------------------------------------------------------------------------------------------
// One 64-pixel chunk of 16 hypotheses: 12 MFMAs, then three phases on the VALU.
//   1. packed over HYPOTHESIS pairs (adjacent MFMA output registers): iz = 1 / zc, du = pu + nx iz, dv = pv + ny iz, q = du^2 + dv^2.
//      nx / ny are the NEGATED camera-frame x / y (the A rows carry the sign, so that no negation is left in the loop).
//   2. e[r][m] = min(sqrt(q), clamp): scalar operations, which write each result straight into the register it is stored from
//      (ev[r] = 4 consecutive pixels of hypothesis r, one dwordx4) -- the 4 x 4 transpose between the two packings costs nothing.
//   3. soft-inlier sigmoid packed over PIXEL pairs of one hypothesis, accumulated per hypothesis.
// Z == 0 detection of the fast path: zacc accumulates iz^2 -- rcp(0) = inf sticks (as would a NaN), anything finite stays finite unless
// |z| < 5e-20, which only sends the wave down the (always exact) slow path once more.
// The low parts of the pose records through the matrix core as well (k2_flags bit 27): per 1 024 pairs twelve v_mfma_f32_16x16x16_f16 chained through
// the accumulator of the fp32 ones, D = A_lo 2^16 . B 2^-16 + (A_hi . B).  Only the k = 0..3 slice of the 16-deep fp16 product is used (the operands of the
// lanes 16..63 are zero).  What it removes is the SYSTEMATIC part of the fast form's error -- the fp32 rounding of a hypothesis' record shifts all of its
// projections the same way, which is 96 % of its score error; the correction (<= half an ulp of the record times the coordinate)
// is often below the ulp of the sum it is added to, and survives in expectation, which is all a sum over 300 000 cells needs.
struct LoOps { h4 x, y, z; };
template <bool EXACT_Z, bool SOFT, bool LO = false>
DM_INLINE bool hp_chunk(float ax, float ay, float az, const float (&Bm)[4], const f2 (&ppix)[4], float clampv, float kA, float kB, f4 (&ev)[4],
                        f2 (&sloc)[4], const LoOps* lo = nullptr, const h4* B16 = nullptr) {
    const f4 z4 = {0.f, 0.f, 0.f, 0.f};
    f2 qq[4][2];
    f2 zacc = splat(0.f);
#pragma unroll
    for (int m = 0; m < 4; m++) {
        // LO: the correction FIRST, as the accumulator the fp32 products are added onto.  The other order loses it: a finished fp32 sum sits on its grid, and
        // adding less than half an ulp returns the same number every time (measured: only 60 % of the error gone); added to the exact first product inside
        // the fused multiply-add it shifts the value BEFORE the rounding, which then keeps it in expectation
        f4 cx4 = z4, cy4 = z4, cz4 = z4;
        if (LO) {
            cx4 = __builtin_amdgcn_mfma_f32_16x16x16f16(lo->x, B16[m], z4, 0, 0, 0);
            cy4 = __builtin_amdgcn_mfma_f32_16x16x16f16(lo->y, B16[m], z4, 0, 0, 0);
            cz4 = __builtin_amdgcn_mfma_f32_16x16x16f16(lo->z, B16[m], z4, 0, 0, 0);
        }
        const f4 nx = __builtin_amdgcn_mfma_f32_16x16x4f32(ax, Bm[m], cx4, 0, 0, 0);
        const f4 ny = __builtin_amdgcn_mfma_f32_16x16x4f32(ay, Bm[m], cy4, 0, 0, 0);
        const f4 dz = __builtin_amdgcn_mfma_f32_16x16x4f32(az, Bm[m], cz4, 0, 0, 0);
#pragma unroll
        for (int pr = 0; pr < 2; pr++) {
            const f2 x = pr ? f2{nx.z, nx.w} : f2{nx.x, nx.y};
            const f2 y = pr ? f2{ny.z, ny.w} : f2{ny.x, ny.y};
            const f2 z = pr ? f2{dz.z, dz.w} : f2{dz.x, dz.y};
            f2 iz = {__builtin_amdgcn_rcpf(z.x), __builtin_amdgcn_rcpf(z.y)};
            if (EXACT_Z) {  // projectPoints: z = Z ? 1/Z : 1
                iz.x = (z.x == 0.0f) ? 1.0f : iz.x;
                iz.y = (z.y == 0.0f) ? 1.0f : iz.y;
            } else {
                zacc = pk_fma(iz, iz, zacc);
            }
            const f2 du = pk_fma(x, iz, splat(ppix[m].x));
            const f2 dv = pk_fma(y, iz, splat(ppix[m].y));
            qq[m][pr] = pk_fma(dv, dv, du * du);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int pr = r >> 1;
        ev[r].x = fminf(__builtin_amdgcn_sqrtf((r & 1) ? qq[0][pr].y : qq[0][pr].x), clampv);
        ev[r].y = fminf(__builtin_amdgcn_sqrtf((r & 1) ? qq[1][pr].y : qq[1][pr].x), clampv);
        ev[r].z = fminf(__builtin_amdgcn_sqrtf((r & 1) ? qq[2][pr].y : qq[2][pr].x), clampv);
        ev[r].w = fminf(__builtin_amdgcn_sqrtf((r & 1) ? qq[3][pr].y : qq[3][pr].x), clampv);
        if (SOFT) sloc[r] = soft_inlier2(f2{ev[r].x, ev[r].y}, kA, kB) + soft_inlier2(f2{ev[r].z, ev[r].w}, kA, kB);
    }
    return EXACT_Z ? false : !(zacc.x + zacc.y <= 3.0e38f);
}

// The exact-transform chunk (round 6, k2_flags bit 28): hp_chunk with E = R.X + t from the split records (k_pose_prep_split) -- per row one K = 32 fp16 MFMA
// for the cross terms, one K = 16 fp16 MFMA for the exactly summed high products (its B operand is the first half of the other's), one packed fma per
// register pair for E = D_hi + 2^-14 D_cross: the camera-frame point is rounded to float ONCE.  Then hp_chunk's tail with one Newton step on v_rcp_f32:
// the hardware reciprocal's error is not zero-mean, and a biased 1 / z scales every projection of a hypothesis about the principal point the same way --
// measured (scripts/r06_k2_diag.py, profiles/r06_k2_diag.txt): with an exact E and the plain v_rcp_f32 the softmax weight of two unrelated hypotheses in a tie is
// still off by 5.7e-4 (stated 1e-4), with the Newton step by 5.3e-5; max |err - oracle| over all cells 7.6e-5 px.
struct ExOps { h8 cx, cy, cz; h4 hx, hy, hz; };
// E = D_hi + 2^-14 D_cross on a register pair of the two accumulators.  (Spelled out as inline assembly -- the compiler emits half of these as two
// v_fma_f32 each -- it returned garbage: the hazard recogniser does not see an asm statement's read of a matrix-core result, and gfx950 has no interlock there.)
DM_INLINE f2 ex_combine(f2 c, f2 k, f2 h) { return pk_fma(c, k, h); }
// RSQ (EXF = 2): the tail without the reciprocal of z.  With nu = pu z - xc, nv = pv z - yc (one fma each on the once-rounded point):
//   e = sqrt(nu^2 + nv^2) / |z| = n rsq(n z^2),  n = nu^2 + nv^2
// -- ONE transcendental for reciprocal, Newton step and square root (3 instead of 4 per pair with the sigmoid's two; transcendentals are a third of the
// kernel's issue cycles).  v_rsq_f32's error does not bias a hypothesis against another the way v_rcp_f32's did: its argument n z^2 spreads over many octaves
// within every hypothesis (the reciprocal's argument z sits within two), so what is systematic in it is common to all.  z == 0 (and an exactly zero residual):
// the argument is 0, rsq = inf, which sticks in the accumulated products and sends the chunk down the exact-z path as before.
template <bool EXACT_Z, bool SOFT, bool RSQ = false>
DM_INLINE bool hp_chunk_ex(const ExOps& A, const h8 (&B8)[4], const f2 (&ppix)[4], float clampv, float kA, float kB, f4 (&ev)[4], f2 (&sloc)[4]) {
    const f4 z4 = {0.f, 0.f, 0.f, 0.f};
    const f2 k10 = splat(6.103515625e-05f);  // 2^-14: the cross group's scale
    constexpr bool TAIL_RSQ = RSQ && !EXACT_Z;
    f2 qq[4][2];
    f2 zacc = splat(0.f);
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const h4 b4 = __builtin_shufflevector(B8[m], B8[m], 0, 1, 2, 3);
        const f4 cx = __builtin_amdgcn_mfma_f32_16x16x32_f16(A.cx, B8[m], z4, 0, 0, 0);
        const f4 cy = __builtin_amdgcn_mfma_f32_16x16x32_f16(A.cy, B8[m], z4, 0, 0, 0);
        const f4 cz = __builtin_amdgcn_mfma_f32_16x16x32_f16(A.cz, B8[m], z4, 0, 0, 0);
        const f4 hx = __builtin_amdgcn_mfma_f32_16x16x16f16(A.hx, b4, z4, 0, 0, 0);
        const f4 hy = __builtin_amdgcn_mfma_f32_16x16x16f16(A.hy, b4, z4, 0, 0, 0);
        const f4 hz = __builtin_amdgcn_mfma_f32_16x16x16f16(A.hz, b4, z4, 0, 0, 0);
        f2 iz0 = splat(0.f);
#pragma unroll
        for (int pr = 0; pr < 2; pr++) {
            const f2 x = ex_combine(pr ? f2{cx.z, cx.w} : f2{cx.x, cx.y}, k10, pr ? f2{hx.z, hx.w} : f2{hx.x, hx.y});
            const f2 y = ex_combine(pr ? f2{cy.z, cy.w} : f2{cy.x, cy.y}, k10, pr ? f2{hy.z, hy.w} : f2{hy.x, hy.y});
            const f2 z = ex_combine(pr ? f2{cz.z, cz.w} : f2{cz.x, cz.y}, k10, pr ? f2{hz.z, hz.w} : f2{hz.x, hz.y});
            if (TAIL_RSQ) {
                const f2 nu = pk_fma(splat(ppix[m].x), z, x), nv = pk_fma(splat(ppix[m].y), z, y);  // x, y carry -xc, -yc
                const f2 n = pk_fma(nv, nv, nu * nu);
                const f2 arg = n * (z * z);
                const f2 r = {__builtin_amdgcn_rsqf(arg.x), __builtin_amdgcn_rsqf(arg.y)};
                if (pr == 0) iz0 = r; else zacc = pk_fma(iz0, r, zacc);
                qq[m][pr] = n * r;  // the distance itself
                continue;
            }
            f2 iz = {__builtin_amdgcn_rcpf(z.x), __builtin_amdgcn_rcpf(z.y)};
            iz = pk_fma(pk_fma(-z, iz, splat(1.0f)), iz, iz);  // z == 0: inf -> NaN, which sticks in zacc like the inf of the plain form
            if (EXACT_Z) {  // projectPoints: z = Z ? 1/Z : 1
                iz.x = (z.x == 0.0f) ? 1.0f : iz.x;
                iz.y = (z.y == 0.0f) ? 1.0f : iz.y;
            } else if (pr == 0) {
                iz0 = iz;
            } else {
                zacc = pk_fma(iz0, iz, zacc);  // one fma for both register pairs of an m: a NaN or an inf in either survives the product (inf x 0 = NaN)
            }
            const f2 du = pk_fma(x, iz, splat(ppix[m].x));
            const f2 dv = pk_fma(y, iz, splat(ppix[m].y));
            qq[m][pr] = pk_fma(dv, dv, du * du);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int pr = r >> 1;
        const float q0 = (r & 1) ? qq[0][pr].y : qq[0][pr].x, q1 = (r & 1) ? qq[1][pr].y : qq[1][pr].x;
        const float q2 = (r & 1) ? qq[2][pr].y : qq[2][pr].x, q3 = (r & 1) ? qq[3][pr].y : qq[3][pr].x;
        ev[r].x = fminf(TAIL_RSQ ? q0 : __builtin_amdgcn_sqrtf(q0), clampv);
        ev[r].y = fminf(TAIL_RSQ ? q1 : __builtin_amdgcn_sqrtf(q1), clampv);
        ev[r].z = fminf(TAIL_RSQ ? q2 : __builtin_amdgcn_sqrtf(q2), clampv);
        ev[r].w = fminf(TAIL_RSQ ? q3 : __builtin_amdgcn_sqrtf(q3), clampv);
        if (SOFT) sloc[r] = soft_inlier2(f2{ev[r].x, ev[r].y}, kA, kB) + soft_inlier2(f2{ev[r].z, ev[r].w}, kA, kB);
    }
    return EXACT_Z ? false : !(fabsf(zacc.x + zacc.y) <= 3.0e38f);  // products of two reciprocals: -inf counts as well
}

// The B operand of hp_chunk_ex for one (chunk, m): lane (g, c) holds coordinate g of pixel 4c + m (g = 3: the constants the translation pieces multiply).
// X = XT + XA' + XM + XL1 + XL2 (k_pose_prep_split); every remainder below is exact in fp32.  oor: |X| >= 2^16 mm (or NaN).
// Conversions round to nearest (v_cvt_pk_f16_f32): every piece but XL2 is exactly representable, and XL2 must not be TRUNCATED -- the budget for a systematic
// error of the camera-frame point is ~1e-6 mm (k_pose_prep_split).
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
DM_INLINE unsigned pk_h2(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_convertvector(f2{a, b}, h2v)); }
// two floats as two bfloat16 in a dword, each rounded to nearest even (v_cvt_pk_bf16_f32 on gfx950; NaN stays NaN): the error images of dsac_reproject_bf16
typedef __bf16 b2v __attribute__((ext_vector_type(2)));
DM_INLINE unsigned pk_b2(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_convertvector(f2{a, b}, b2v)); }
// the packer of the 16-bit stores by element type
template <bool BF> DM_INLINE unsigned pk_e2(float a, float b) { if constexpr (BF) return pk_b2(a, b); else return pk_h2(a, b); }
// The lanes of quarter 3 (the translation) run the same code on the constant SPLIT_T_COORD = 2^15 + 1, whose pieces are the powers of two
// (2^10, 2^3, 2^11, 0, 0, 0, 1, 0) that the translation pieces of k_pose_prep_split are scaled against -- no select between coordinates and constants.
constexpr float SPLIT_T_COORD = 32769.0f;
DM_INLINE h8 split_B(float X, bool& oor) {
    const float kt = __builtin_rintf(X * 0.0009765625f);      // XT / 1024
    const float r1 = fmaf(-1024.f, kt, X);                     // X - XT, |.| <= 512
    const float ka = __builtin_rintf(r1 * 0.03125f);           // XA' / 32
    const float r2 = fmaf(-32.f, ka, r1);                      // X - XA, |.| <= 16
    const float xm = __builtin_rintf(r2);                      // XM
    const float xl = r2 - xm;                                  // |.| <= 0.5
    const float kl = __builtin_rintf(xl * 4096.f);             // XL1 2^12
    const float xl2 = fmaf(-0.000244140625f, kl, xl);          // XL2
    const float ja = fmaf(32.f, kt, ka);                       // XA / 32
    oor = oor || !(fabsf(ja) <= 2047.f);
    const u4v v = {pk_h2(ja, xm * 8.f), pk_h2(kt * 64.f, kl * 0.25f), pk_h2(xl2 * 1024.f, ka * 32.f), pk_h2(xm, kl * 0.000244140625f)};
    return __builtin_bit_cast(h8, v);
}

template <int HT, bool ERR, bool SOFT, bool UV, int KM_CH>
__global__ __launch_bounds__(K2_THREADS) void k_reproject_hp(const float* __restrict__ staged, const float* __restrict__ xyz,
                                                             const float* __restrict__ uv, float* __restrict__ err,
                                                             float* __restrict__ soft_part, int N, int P, int W, int PT, int NT, float cx,
                                                             float cy, float clampv, float kA, float kB, int kflags, int Nf,
                                                             long long xyz_stride, long long uv_stride) {
    static_assert(HT % 16 == 0, "hypothesis tile must be a multiple of 16");
    const int b = blockIdx.x;
    const int q = b >> 3;
    int ht, pt;  // block order as in k_reproject (NT > 0: hypothesis tiles innermost; NT < 0: pixel tiles innermost)
    if (NT > 0) { ht = q % NT; pt = (q / NT) * 8 + (b & 7); }
    else { const int PTG = (PT + 7) >> 3; ht = q / PTG; pt = (q % PTG) * 8 + (b & 7); }
    if (pt >= PT) return;
    const int h0 = ht * HT;
    const int nh = min(HT, N - h0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    {   // frame batch: all hypotheses of this tile score the same frame (Nf is a multiple of HT)
        const int frame = h0 / Nf;
        xyz += (long long)frame * xyz_stride;
        if (UV) uv += (long long)frame * uv_stride;
    }

    // A operands in MFMA lane order: s_A[(gi*3 + comp)*64 + l] = record[h0 + 16 gi + l%16][comp][k = l/16]; hypotheses beyond the
    // ragged end repeat the last valid one (their results are never stored, and a zero record would send every wave down the Z == 0 path)
    __shared__ float s_A[(HT / 16) * 3 * 64];
    __shared__ float s_soft[SOFT ? (K2_THREADS / 64) * HT : 1];
    for (int i = tid; i < (HT / 16) * 3 * 64; i += K2_THREADS) {
        const int l = i & 63, cg = i >> 6;
        const int comp = cg % 3, gi = cg / 3;
        const int hyp = min(16 * gi + (l & 15), nh - 1), k = l >> 4;
        const float v = staged[(size_t)(h0 + hyp) * POSE_STRIDE + comp * 4 + k];
        s_A[i] = comp < 2 ? -v : v;  // x and y rows negated: the MFMA yields (-xc, -yc, zc), du = pu + (-xc) / zc needs no sign flip
    }

    float Bm[KM_CH][4];
    f2 ppix[KM_CH][4];
    int p0[KM_CH];
    bool valid[KM_CH];
#pragma unroll
    for (int ch = 0; ch < KM_CH; ch++) {
        const int chunk0 = (pt * (K2_THREADS / 64) * KM_CH + wave * KM_CH + ch) * 64;
        p0[ch] = chunk0 + 4 * c;       // this lane's 4 consecutive pixels
        valid[ch] = p0[ch] < P;        // P % 4 == 0
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int pc = min(p0[ch] + m, P - 1);
            Bm[ch][m] = (g < 3) ? xyz[(size_t)pc * 3 + g] : 1.0f;
        }
        if (UV) {
            if (valid[ch]) {
                const f4* su = reinterpret_cast<const f4*>(uv + (size_t)p0[ch] * 2);
                const f4 u0 = su[0], u1 = su[1];
                ppix[ch][0] = f2{u0.x - cx, u0.y - cy}; ppix[ch][1] = f2{u0.z - cx, u0.w - cy};
                ppix[ch][2] = f2{u1.x - cx, u1.y - cy}; ppix[ch][3] = f2{u1.z - cx, u1.w - cy};
            } else {
                ppix[ch][0] = ppix[ch][1] = ppix[ch][2] = ppix[ch][3] = splat(0.f);
            }
        } else {
            int y = p0[ch] / W, x = p0[ch] - y * W;  // implicit grid: one integer division per chunk, then walk (with row wrap)
#pragma unroll
            for (int m = 0; m < 4; m++) {
                ppix[ch][m] = f2{(float)x - cx, (float)y - cy};
                if (++x == W) { x = 0; y++; }
            }
        }
    }
    __syncthreads();

    for (int gi = 0; gi < HT / 16; gi++) {
        if (16 * gi >= nh) break;
        const float ax = s_A[(gi * 3 + 0) * 64 + lane], ay = s_A[(gi * 3 + 1) * 64 + lane], az = s_A[(gi * 3 + 2) * 64 + lane];
        const int hyp0 = 16 * gi + 4 * g;  // this lane's 4 hypotheses: hyp0 .. hyp0 + 3
        f2 ssum[4] = {splat(0.f), splat(0.f), splat(0.f), splat(0.f)};
#pragma unroll
        for (int ch = 0; ch < KM_CH; ch++) {
            f4 ev[4];  // ev[r] = 4 consecutive pixels of hypothesis hyp0 + r
            f2 sloc[4];
            if (kflags & 2) {  // measurement knob (k2_flags bit 1): the store schedule alone, no arithmetic -- the ceiling of this write pattern
                if (ERR && valid[ch]) {
                    f4* dst = reinterpret_cast<f4*>(err + (size_t)(h0 + hyp0) * P + p0[ch]);
                    const size_t rs = (size_t)P / 4;
                    const f4 o = {ax, ay, az, (float)gi};
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if (hyp0 + r >= nh) continue;
                        f4* q = dst + r * rs;
                        const int mode = (kflags >> 2) & 7;  // cache policy of the store (measurement): 0 nt, 1 plain, 2 sc1, 3 sc0 sc1, 4 nt sc1, 5 sc0
                        if (mode == 0) __builtin_nontemporal_store(o, q);
                        else if (mode == 1) *q = o;
                        else if (mode == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(q), "v"(o) : "memory");
                        else if (mode == 3) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(q), "v"(o) : "memory");
                        else if (mode == 4) asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" ::"v"(q), "v"(o) : "memory");
                        else asm volatile("global_store_dwordx4 %0, %1, off sc0" ::"v"(q), "v"(o) : "memory");
                    }
                }
                continue;
            }
            // projectPoints' "z = Z ? 1/Z : 1": one test for the 16 pairs, wave-uniform slow path (practically never) that redoes the chunk
            if (__builtin_expect(__any(hp_chunk<false, SOFT>(ax, ay, az, Bm[ch], ppix[ch], clampv, kA, kB, ev, sloc)), 0))
                (void)hp_chunk<true, SOFT>(ax, ay, az, Bm[ch], ppix[ch], clampv, kA, kB, ev, sloc);
            if (SOFT) {
                const f2 vf = splat(valid[ch] ? 1.0f : 0.0f);
#pragma unroll
                for (int r = 0; r < 4; r++) ssum[r] = pk_fma(sloc[r], vf, ssum[r]);
            }
            if (ERR && valid[ch]) {
                f4* dst = reinterpret_cast<f4*>(err + (size_t)(h0 + hyp0) * P + p0[ch]);
                const size_t rs = (size_t)P / 4;  // row stride in f4 (P % 4 == 0)
                if (nh == HT) {  // full tile (uniform): no per-row guards
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if (kflags & 1) dst[r * rs] = ev[r]; else __builtin_nontemporal_store(ev[r], dst + r * rs);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if (hyp0 + r < nh) { if (kflags & 1) dst[r * rs] = ev[r]; else __builtin_nontemporal_store(ev[r], dst + r * rs); }
                    }
                }
            }
        }
        if (SOFT) {
            // the 16 lanes of a DPP row hold the same 4 hypotheses
            const float s0 = row16_sum(ssum[0].x + ssum[0].y), s1 = row16_sum(ssum[1].x + ssum[1].y);
            const float s2 = row16_sum(ssum[2].x + ssum[2].y), s3 = row16_sum(ssum[3].x + ssum[3].y);
            if (c == 0) {  // written exactly once per (wave, hypothesis)
                float* dst = s_soft + wave * HT + hyp0;
                if (hyp0 + 0 < nh) dst[0] = s0;
                if (hyp0 + 1 < nh) dst[1] = s1;
                if (hyp0 + 2 < nh) dst[2] = s2;
                if (hyp0 + 3 < nh) dst[3] = s3;
            }
        }
    }

    if (SOFT) {
        __syncthreads();
        if (tid < nh) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < K2_THREADS / 64; w++) s += s_soft[w * HT + tid];
            soft_part[(size_t)pt * N + h0 + tid] = s;
        }
    }
}

template <int HT, int KM_CH>
static hipError_t launch_reproject_hp(hipStream_t st, int N, const float* staged, const FrameDev& F, float clampv, float* err, float kA,
                                      float kB, float* soft_part, int Nf, bool pixel_minor, int kflags, hipEvent_t evA, hipEvent_t evB) {
    const int tile = K2_THREADS * KM_CH;  // 64 pixels per wave-chunk
    const int PT = (F.P + tile - 1) / tile;
    const int NTa = (N + HT - 1) / HT;
    const int grid = ((PT + 7) / 8) * 8 * NTa;
    const int NT = pixel_minor ? -NTa : NTa;
    const bool ERR = err != nullptr, SOFT = soft_part != nullptr, UV = F.uv != nullptr;
    // experiment knob (k2_flags bits 8..15): that many 8-KiB units of unused dynamic LDS per workgroup cap the workgroups per CU
    const size_t lds_pad = (size_t)((kflags >> 8) & 0xff) * 8192;
#define DSAC_K2H(E, S, U)                                                                                                             \
    hipExtLaunchKernelGGL((k_reproject_hp<HT, E, S, U, KM_CH>), dim3(grid), dim3(K2_THREADS), lds_pad, st, evA, evB, 0, staged, F.xyz, F.uv, err,   \
                          soft_part, N, F.P, F.W, PT, NT, F.cx, F.cy, clampv, kA, kB, kflags, Nf, F.xyz_stride, F.uv_stride)
    if (ERR && SOFT) { if (UV) DSAC_K2H(true, true, true); else DSAC_K2H(true, true, false); }
    else if (ERR) { if (UV) DSAC_K2H(true, false, true); else DSAC_K2H(true, false, false); }
    else if (SOFT) { if (UV) DSAC_K2H(false, true, true); else DSAC_K2H(false, true, false); }
#undef DSAC_K2H
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------
// K2, streaming small-tile form (round 3).  Same arithmetic as k_reproject_hp (hp_chunk), other schedule.
// What decides the store rate of the N x P volume is how many error-image ROWS are open at once across the chip
// (scripts/micro/store_sched.hip, profiles/r03_store_sched.txt: one row 6.9 TB/s, ~30 rows 6.6, ~110 rows 5.8, ~450 rows 5.5):
//   open rows ~ hypotheses per workgroup x (resident waves x pixels a wave holds while it lives) / P.
// So the tile is small (NG x 16 hypotheses, WAVES x CHW x 64 pixels) and its workgroups short-lived, and the per-workgroup set-up
// that made round 2's small tiles lose is cut down: the MFMA A operands come straight from the staged records (one dword per lane and
// component, L2-resident -- no LDS image, no barrier before the first MFMA), the pixel positions of the implicit grid from a
// wave-uniform row / column (W % 64 == 0), and the only barrier is the one before the 16 NG partial soft sums leave the workgroup.
// --------------------------------------------------------------------------------------------------
// ANY (the any-map build of the exact form): no 16-byte alignment of err / uv / xyz and no P % 4 == 0, the same arithmetic per cell.
//   ANY = 1, the main launch: the vector build's code on every lane whose four cells exist -- a 16-byte buffer store and a 16-byte load need dword alignment only
//            on this hardware, so the stores are the very same instructions and the sampled positions are read through a 4-byte-aligned vector type.  A lane that
//            holds the map's last 1-3 cells is left out here (no store, no sigmoid).  Nothing else differs, so the register allocation is the vector build's
//            (handling the last cells inside this kernel was built first: the <64, 256> err + soft instantiations spilled 60-460 bytes per lane).
//            (Four dword stores per lane instead of the one 16-byte store were measured as a build of their own and removed: 562.6 against 169.5 us for
//            256 x 641x479, 10 445 against 2 687 us for 16 x 256, profiles/k2_anymap_ab.txt.)
//   ANY = 2, the tail launch (only when P % 4 != 0): one wave per hypothesis tile on the map's LAST 64-cell chunk, for that one lane alone -- its cells loaded,
//            stored and summed one by one (per-cell validity: a padded cell never adds a sigmoid to a score), its sums in a partial row of their own.
typedef f4 f4_a4 __attribute__((aligned(4)));
// The store of the half-precision build (k_reproject_st<.., EXF = 3 / 4>, dsac_reproject_f16): ev[r] = 4 consecutive cells of row r of the lane's four rows, each
// value rounded to binary16 to nearest even (a plain conversion: the compiler's v_cvt_pk_f16_f32), P % 8 == 0.  base: the group's first row (wave-uniform);
// full (wave-uniform): the hypothesis tile is whole, no test per row; else rows = how many of the lane's four rows exist.  The row stepping is the float build's: a scalar resource, a scalar row offset, a 32-bit lane offset.
//   LAYOUT 1: four 8-byte stores per lane and chunk (a wave store is 4 rows x 128 B)
//   LAYOUT 2: lanes c and c ^ 1 hold cells 8k .. 8k + 3 and 8k + 4 .. 8k + 7 of the same four rows (both exist or neither).  The even lane takes rows 0 and 1 of
//             all eight cells, the odd lane rows 2 and 3: every dword of a stored row is the lane's own or its neighbour's (quad_perm [1, 0, 3, 2]), one select
//             each; two 16-byte stores per lane and chunk
// BF: the values are rounded to bfloat16 instead (k_reproject_st<.., EXF = 5 / 6>, dsac_reproject_bf16) -- only the packing of two floats into a dword differs; the
// lane exchange and the stores move packed dwords and are the same code
typedef unsigned u2v __attribute__((ext_vector_type(2)));
// The stores of a chunk in the full-tile path stand between two scheduling fences, with four idle cycles behind the last one, so that no vector instruction
// WRITES a store's data register right behind the store.  Observed on MI355X (the <64, 64> tile, 64 x 640x480): with `buffer_store_dwordx4 v[32:35], .., s41 offen`
// followed at once by `v_mov_b32 v32, ..` (the partial sums taking over the row's registers) the stored row held the NEW v32 in lanes 12-15 of every row of 16,
// in a few chunks per launch and other ones every run; with the fence, never.  Supposed, not proven: the store reads its data over several cycles.  The
// compiler's hazard table (one idle cycle behind a store of more than 8 bytes) exempts the buffer form with a scalar row offset as free of the hazard, and the
// general path runs with such writes one and two cycles behind 16-bit stores without a failing test ("Wrong rows in the first build").
DM_INLINE void k2_stores_begin() { __builtin_amdgcn_sched_barrier(0); }
DM_INLINE void k2_stores_end() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 3");
    __builtin_amdgcn_sched_barrier(0);
}
template <int LAYOUT, bool BF = false, bool FENCE = false>
DM_INLINE void store_rows_h16(_Float16* base, const f4 (&ev)[4], int P, int p0, int g, int c, bool full, int rows) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0xffffffffu, 0x00020000);
    unsigned pk[4][2];
#pragma unroll
    for (int r = 0; r < 4; r++) { pk[r][0] = pk_e2<BF>(ev[r].x, ev[r].y); pk[r][1] = pk_e2<BF>(ev[r].z, ev[r].w); }
    if constexpr (LAYOUT == 1) {
        const unsigned loff = ((unsigned)(4 * g) * (unsigned)P + (unsigned)p0) * 2u;
        if (full) {
            if (FENCE) k2_stores_begin();
#pragma unroll
            for (int r = 0; r < 4; r++) __builtin_amdgcn_raw_buffer_store_b64(u2v{pk[r][0], pk[r][1]}, rsrc, loff, (unsigned)r * (unsigned)P * 2u, 2);
            if (FENCE) k2_stores_end();
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (r < rows) __builtin_amdgcn_raw_buffer_store_b64(u2v{pk[r][0], pk[r][1]}, rsrc, loff, (unsigned)r * (unsigned)P * 2u, 2);
        }
    } else {
        const bool odd = (c & 1) != 0;
        auto nb = [](unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true); };
        // the neighbour's dwords are fetched by every lane of the pair BEFORE the selects: a cross-lane read under a condition on the lane's parity would find
        // its source lane switched off
        unsigned nk[4][2];
#pragma unroll
        for (int r = 0; r < 4; r++) { nk[r][0] = nb(pk[r][0]); nk[r][1] = nb(pk[r][1]); }
        const u4v ra = {odd ? nk[2][0] : pk[0][0], odd ? nk[2][1] : pk[0][1], odd ? pk[2][0] : nk[0][0], odd ? pk[2][1] : nk[0][1]};
        const u4v rb = {odd ? nk[3][0] : pk[1][0], odd ? nk[3][1] : pk[1][1], odd ? pk[3][0] : nk[1][0], odd ? pk[3][1] : nk[1][1]};
        const int r0 = odd ? 2 : 0;  // this lane's rows: r0, r0 + 1
        const unsigned loff = ((unsigned)(4 * g + r0) * (unsigned)P + (unsigned)(p0 & ~7)) * 2u;
        if (full) {
            if (FENCE) k2_stores_begin();
            __builtin_amdgcn_raw_buffer_store_b128(ra, rsrc, loff, 0u, 2);
            __builtin_amdgcn_raw_buffer_store_b128(rb, rsrc, loff, (unsigned)P * 2u, 2);
            if (FENCE) k2_stores_end();
        } else {
            if (r0 < rows) __builtin_amdgcn_raw_buffer_store_b128(ra, rsrc, loff, 0u, 2);
            if (r0 + 1 < rows) __builtin_amdgcn_raw_buffer_store_b128(rb, rsrc, loff, (unsigned)P * 2u, 2);
        }
    }
}
// The immediate of s_waitcnt on gfx9 for "at most n vector memory operations (loads AND stores: one counter) in flight", the other counters not waited for:
// vmcnt[3:0] in bits 3:0, vmcnt[5:4] in bits 15:14; expcnt (bits 6:4) and lgkmcnt (bits 11:8) at their maxima
constexpr int k2_vmcnt_imm(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0f70; }
template <int NG, int CHW, int WAVES, bool PW, bool ERR, bool SOFT, bool UV, bool G64, int MINW, bool LO = false, int EXF = 0, int ANY = 0>
__global__ __launch_bounds__(WAVES * 64, MINW) void k_reproject_st(const float* __restrict__ staged, const float* __restrict__ xyz,
                                                             const float* __restrict__ uv, float* __restrict__ err,
                                                             float* __restrict__ soft_part, int N, int P, int W, int PT, float cx, float cy,
                                                             float clampv, float kA, float kB, int kflags, int Nf, long long xyz_stride,
                                                             long long uv_stride, const float* __restrict__ staged_lo = nullptr,
                                                             const void* __restrict__ split = nullptr, const float4* __restrict__ cams = nullptr) {
    constexpr int HT = 16 * NG;
    constexpr bool EX = EXF != 0, RSQ = EXF >= 2;  // EXF: 0 = fp32 transform, 1 = exact transform (split fp16 records), 2 = the same with the one-transcendental tail (hp_chunk_ex)
    // EXF = 3 / 4: EXF = 2 with the error images stored as IEEE binary16 (dsac_reproject_f16; `err` then points to halves).  Everything up to ev[r] and the sigmoid
    // sums is EXF = 2's code; only the store differs: 3 = four 8-byte stores per lane and chunk, 4 = lanes c and c ^ 1 trade rows, two 16-byte stores of 8 cells each.
    // The element type rides in EXF and not in a parameter of its own so that the float kernels keep their names (the Makefile's ISA-mix targets select by name)
    // EXF = 5 / 6: the same two store layouts with the values rounded to bfloat16 (dsac_reproject_bf16): 5 = layout 1, 6 = layout 2
    constexpr bool BF16 = EXF >= 5;
    constexpr int H16 = EXF >= 5 ? EXF - 4 : EXF >= 3 ? EXF - 2 : 0;
    static_assert(H16 == 0 || (ERR && ANY == 0 && !LO), "half error images: the vector build of the exact form, with an error image to store");
    const int b = blockIdx.x;
    int ht, pt;
    if (kflags & 32) { pt = b % PT; ht = b / PT; }  // plain pixel-minor order
    else if (WAVES == 1) {
        // one-wave workgroups, XCD-aware: the four workgroups b, b + 8, b + 16, b + 24 (same XCD, dispatched back to back) take four ADJACENT
        // 64-pixel chunks, so that an XCD still writes 1 KiB runs of every row
        const int q = b >> 5, sub = (b >> 3) & 3, PTG = (PT + 31) >> 5;
        ht = q / PTG;
        pt = ((q % PTG) * 8 + (b & 7)) * 4 + sub;
        if (pt >= PT) return;
    } else {  // XCD-aware pixel-minor order (block b -> XCD b % 8 keeps its eighth of the pixel tiles)
        const int q = b >> 3, PTG = (PT + 7) >> 3;
        ht = q / PTG;
        pt = (q % PTG) * 8 + (b & 7);
        if (pt >= PT) return;
    }
    // The hypothesis walk (k2_plan.h, K2Plan::hyp_walk; k2_flags bits 6-7 hold its log2, set by dk::reproject alone): the builds with the full-tile path score
    // HB consecutive hypothesis tiles of one frame on the workgroup's pixel tile -- the coordinate loads, their fp16 split and the prologue's wait happen once
    // per walk.  `ht` counts walks; the plan allows HB > 1 only where every tile of every walk is whole and no walk straddles a frame.  Every other build: HB = 1
    constexpr bool FULL_TILE = EXF >= 2 && ANY == 0 && !LO && G64 && !UV && PW && MINW <= 3;
    const int HB = FULL_TILE ? 1 << ((kflags >> K2_KFLAG_WALK_SHIFT) & 3) : 1;
    int h0 = ht * HT * HB;
    int nh = min(HT, N - h0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    {
        const int frame = h0 / Nf;
        xyz += (long long)frame * xyz_stride;
        if (UV) uv += (long long)frame * uv_stride;
        // one camera per frame: the tile's principal point (a scalar load, frame is uniform over the workgroup); the focal length is in the records.  The exact
        // builds only -- per-frame cameras run no other form (api.hip refuses by name), and the fp32 / two-piece builds keep the code they had
        if (EX && cams) {
            const float4 k = cams[frame];
            cx = k.z; cy = k.w;
        }
    }
    __shared__ float s_soft[(SOFT && !PW) ? WAVES * HT : 1];
    // PW: every wave writes its own partial soft sums (row pt * WAVES + wave of soft_part), no LDS, no barrier

    // B operands (coordinate g of pixel 4c + m of every chunk) and the MFMA A operands (x-, y-, z-row entry k = g of hypothesis c)
    // G64 (implicit grid, W % 64 == 0: a 64-pixel chunk never straddles a row): the pixel positions are rebuilt from one (column, row) pair
    // per chunk in front of every use instead of living in 8 registers per chunk
    float Bm[CHW][4];
    f2 ppix[G64 ? 1 : CHW][4];
    // G64: row and first column of a chunk are wave-uniform and live in SCALAR registers (late round 3: as a lane-dependent pair per chunk they
    // were 8 vector registers, exactly what the 128-register build of the <64 hypotheses, 256 pixels> form spilled)
    int sx0[G64 ? CHW : 1];
    float sby[G64 ? CHW : 1];
    int p0[CHW];
    bool valid[CHW];
    const int chunk0 = (pt * WAVES + wave) * CHW + (ANY == 2 ? (P - 1) >> 6 : 0);  // the tail launch: the map's last chunk
#pragma unroll
    for (int ch = 0; ch < CHW; ch++) {
        p0[ch] = (chunk0 + ch) * 64 + 4 * c;
        if constexpr (ANY == 1) valid[ch] = p0[ch] + 3 < P;                      // all four cells exist
        else if constexpr (ANY == 2) valid[ch] = p0[ch] < P && p0[ch] + 3 >= P;  // the lane of the map's last 1-3 cells
        else valid[ch] = p0[ch] < P;  // P % 4 == 0
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int pc = min(p0[ch] + m, P - 1);
            Bm[ch][m] = (g < 3) ? xyz[(size_t)pc * 3 + g] : 1.0f;
        }
    }
    // EX: the split fp16 B operands of every (chunk, m); a chunk with a coordinate beyond 2^16 mm takes the fp32 path (wave-uniform flag per chunk)
    h8 B8[EX ? CHW : 1][4];
    bool oor[EX ? CHW : 1];
    if (EX) {
#pragma unroll
        for (int ch = 0; ch < CHW; ch++) {
            bool o = false;
#pragma unroll
            for (int m = 0; m < 4; m++) B8[ch][m] = split_B((g < 3) ? Bm[ch][m] : SPLIT_T_COORD, o);
            oor[ch] = __any(o);
        }
    }
    // LO: the fp16 B operands of every (chunk, m) -- (X, Y, Z, 1) 2^-16 of pixel column c in the lanes of row 0, zero elsewhere.  Row 0 holds X itself;
    // Y and Z come over from rows 1 and 2 with one lane swap each
    h4 B16[LO ? CHW : 1][4];
    if (LO) {
#pragma unroll
        for (int ch = 0; ch < CHW; ch++)
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const unsigned v = __builtin_bit_cast(unsigned, Bm[ch][m]);
                const auto r16 = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // [1]: row 0 <- row 1
                const auto r32 = __builtin_amdgcn_permlane32_swap(v, v, false, false);  // [1]: rows 0, 1 <- rows 2, 3
                const unsigned u16 = r16[1], u32 = r32[1];
                const float s = 1.52587890625e-05f;  // 2^-16
                const float X = Bm[ch][m] * s, Y = __builtin_bit_cast(float, u16) * s, Z = __builtin_bit_cast(float, u32) * s;
                const bool r0 = g == 0;
                // the constant 1 of the translation column travels as 2^-8 (its record entry as lo 2^8): 2^-16 is a SUBNORMAL half, which the matrix core
                // flushes -- measured: with it the translation's correction, the largest of the four, was simply missing
                B16[ch][m] = h4{(_Float16)(r0 ? X : 0.f), (_Float16)(r0 ? Y : 0.f), (_Float16)(r0 ? Z : 0.f), (_Float16)(r0 ? 0.00390625f : 0.f)};
            }
    }
    // A operands: with up to two groups all of them are loaded up front; with four they are fetched one group ahead (two register sets instead of
    // four: the 128-register build of the <64 hypotheses, 256 pixels> form needs the six registers)
    constexpr bool A_AHEAD = NG > 2;
    float ax[EX ? 1 : NG], ay[EX ? 1 : NG], az[EX ? 1 : NG];
    LoOps alo[LO ? NG : 1];
    ExOps aex[EX ? NG : 1];
    // lh, lc: the first hypothesis of the tile load_A fetches for and the lane's column -- h0 and c, but where the walk of the full-tile builds passes copies of
    // them through an empty asm: no operand address then lives across the tiles as an induction variable (vector registers the <64, 256> builds do not have)
    int lh = h0, lc = c;
    auto load_A = [&](int gi) {
        const int hyp = min(16 * gi + lc, nh - 1);  // beyond the ragged end: repeat the last valid hypothesis (never stored)
        if (EX) {
            // the split records in the matrix core's lane layout: quarter g of rows x, y, z of hypothesis c -- 16 bytes (K = 32 operand) + 8 bytes (K = 16) each
            const h8* rc = reinterpret_cast<const h8*>(split) + (size_t)(lh + hyp) * 12 + g;
            const h4* rh = reinterpret_cast<const h4*>(reinterpret_cast<const char*>(split) + (size_t)N * SPLIT_CROSS_BYTES) + (size_t)(lh + hyp) * 12 + g;
            aex[gi].cx = rc[0]; aex[gi].cy = rc[4]; aex[gi].cz = rc[8];
            aex[gi].hx = rh[0]; aex[gi].hy = rh[4]; aex[gi].hz = rh[8];
            return;
        }
        const float* rec = staged + (size_t)(lh + hyp) * POSE_STRIDE + g;
        ax[gi] = rec[0]; ay[gi] = rec[4]; az[gi] = rec[8];
        if (LO) {
            // the records' low parts x 2^16 (x and y rows negated like the high parts), k = 0..3 of hypothesis c in the lanes of row 0
            const f4* rl = reinterpret_cast<const f4*>(staged_lo + (size_t)(lh + hyp) * POSE_STRIDE);
            const float S = (g == 0) ? 65536.f : 0.f, T = (g == 0) ? 256.f : 0.f;  // rotation entries x 2^16 against coordinates x 2^-16, translation x 2^8 against 2^-8
            const f4 lx = rl[0], ly = rl[1], lz = rl[2];
            alo[gi].x = h4{(_Float16)(-lx.x * S), (_Float16)(-lx.y * S), (_Float16)(-lx.z * S), (_Float16)(-lx.w * T)};
            alo[gi].y = h4{(_Float16)(-ly.x * S), (_Float16)(-ly.y * S), (_Float16)(-ly.z * S), (_Float16)(-ly.w * T)};
            alo[gi].z = h4{(_Float16)(lz.x * S), (_Float16)(lz.y * S), (_Float16)(lz.z * S), (_Float16)(lz.w * T)};
        }
    };
#pragma unroll
    for (int gi = 0; gi < (A_AHEAD ? 1 : NG); gi++) load_A(gi);
#pragma unroll
    for (int ch = 0; ch < CHW; ch++) {
        if (UV) {
            constexpr int pc = G64 ? 0 : 1;
            if constexpr (ANY != 0) {
                if (valid[ch]) {
                    f4 u0, u1;
                    if constexpr (ANY != 2) {  // any 4-byte-aligned uv: the same two 16-byte loads with dword alignment
                        const f4_a4* su = reinterpret_cast<const f4_a4*>(uv + (size_t)p0[ch] * 2);
                        u0 = su[0]; u1 = su[1];
                    } else {  // cell by cell; cells beyond the map repeat the last one, as their coordinates do
                        const float* s1 = uv + (size_t)min(p0[ch] + 1, P - 1) * 2;
                        const float* s2 = uv + (size_t)min(p0[ch] + 2, P - 1) * 2;
                        const float* s3 = uv + (size_t)(P - 1) * 2;
                        u0 = f4{uv[(size_t)p0[ch] * 2], uv[(size_t)p0[ch] * 2 + 1], s1[0], s1[1]};
                        u1 = f4{s2[0], s2[1], s3[0], s3[1]};
                    }
                    ppix[ch * pc][0] = f2{u0.x - cx, u0.y - cy}; ppix[ch * pc][1] = f2{u0.z - cx, u0.w - cy};
                    ppix[ch * pc][2] = f2{u1.x - cx, u1.y - cy}; ppix[ch * pc][3] = f2{u1.z - cx, u1.w - cy};
                } else {
                    ppix[ch * pc][0] = ppix[ch * pc][1] = ppix[ch * pc][2] = ppix[ch * pc][3] = splat(0.f);
                }
            } else if (valid[ch]) {
                const f4* su = reinterpret_cast<const f4*>(uv + (size_t)p0[ch] * 2);
                const f4 u0 = su[0], u1 = su[1];
                ppix[ch * pc][0] = f2{u0.x - cx, u0.y - cy}; ppix[ch * pc][1] = f2{u0.z - cx, u0.w - cy};
                ppix[ch * pc][2] = f2{u1.x - cx, u1.y - cy}; ppix[ch * pc][3] = f2{u1.z - cx, u1.w - cy};
            } else {
                ppix[ch * pc][0] = ppix[ch * pc][1] = ppix[ch * pc][2] = ppix[ch * pc][3] = splat(0.f);
            }
        } else if (G64) {
            // row and first column are wave-uniform (scalar division)
            const int cpr = W >> 6;
            const int y = (chunk0 + ch) / cpr, xc0 = ((chunk0 + ch) - y * cpr) * 64;
            sx0[ch] = __builtin_amdgcn_readfirstlane(xc0);
            sby[ch] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (float)y - cy)));
        } else {
            constexpr int pc = G64 ? 0 : 1;
            int y = p0[ch] / W, x = p0[ch] - y * W;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                ppix[ch * pc][m] = f2{(float)x - cx, (float)y - cy};
                if (++x == W) { x = 0; y++; }
            }
        }
    }

    // The full-tile path: the one-transcendental exact vector builds on the implicit grid (the auto policy's kernels for W % 64 == 0, the bench shape among
    // them).  One wave-uniform test picks it: a whole hypothesis tile, every chunk inside the map, no chunk with a coordinate beyond the split's range;
    // k2_flags bit 30 sends every tile down the general path below (the A/B knob).  The calls, their order and operands, the loop nest and the stores are the
    // general path's.  What is left out is every branch the compiler's wait-count analysis cannot follow: the exec-masked skips around a chunk body and its
    // stores (valid[ch], the row guards) and the far-coordinate cold path, which issues loads of its own and comes back by a backward branch.  Over those
    // joins the analysis keeps, for every operand register, the fewest younger memory operations of any path, and loads and stores share one counter: in
    // the general path every chunk top waits until at most 6 (in the last group: none) of the wave's own stores are in flight, for operands that landed
    // long before.  Here the only waits on that counter are the counted ones, which the analysis takes over.
    // (The other exact builds keep the general path alone: with a second path the sampled-position builds, the reciprocal tail and the four-waves-per-SIMD
    // tile spill 50-330 bytes per lane.)
    if constexpr (FULL_TILE) {
        bool far = false;
#pragma unroll
        for (int ch = 0; ch < CHW; ch++) far = far || oor[ch];
        if (nh == HT && (chunk0 + CHW) * 64 <= P && !far && !(kflags & K2_FLAG_GENERAL_PATH)) {
            // error-image stores of one group: what is certainly issued between the fetch of a group's operands and their first use (the four partial-sum
            // stores of the lanes c == 0 sit under a branch and do not count)
            constexpr int GRP_STORES = ERR ? CHW * (H16 == 2 ? 2 : 4) : 0;
            // end of the prologue: every load so far (coordinates, the first group's operands), before the first store -- the first MFMA waits for them anyway
            __builtin_amdgcn_s_waitcnt(k2_vmcnt_imm(0));  // 0x0f70: vmcnt(0)
            // The walk over the HB tiles stays ROLLED (the executed path is about 35 KB of a 64 KB instruction cache).  The fetch one group ahead carries across
            // the tile boundary: the last group of a tile fetches the first group of the next one, and the wait for it stands at the top of the next trip -- the
            // same count as at any group top: the fetch was issued at the top of the last group, the group's GRP_STORES error-image stores behind it
            static_assert(A_AHEAD, "the walk fetches the next tile's first group from the last group of this one");
#pragma unroll 1
            for (int k = 0;; k++) {
                // tile top: the first group's operands, fetched from the last group of the tile before (the first tile's: landed with the prologue's wait)
                __builtin_amdgcn_s_waitcnt(k2_vmcnt_imm(GRP_STORES));
                asm volatile("" : "+v"(aex[0].cx), "+v"(aex[0].cy), "+v"(aex[0].cz), "+v"(aex[0].hx), "+v"(aex[0].hy), "+v"(aex[0].hz));
#pragma unroll
                for (int gi = 0; gi < NG; gi++) {
                    // group top: the operands fetched one group ahead
                    if (A_AHEAD && gi > 0) {
                        __builtin_amdgcn_s_waitcnt(k2_vmcnt_imm(GRP_STORES));  // 16 stores: 0x4f70 = vmcnt(16); 8: 0x0f78; 4: 0x0f74; 2: 0x0f72; none: 0x0f70
                        // the operands pass through here: no MFMA of the group is scheduled in front of the wait (it would get a wait of its own)
                        asm volatile("" : "+v"(aex[gi].cx), "+v"(aex[gi].cy), "+v"(aex[gi].cz), "+v"(aex[gi].hx), "+v"(aex[gi].hy), "+v"(aex[gi].hz));
                    }
                    lh = h0; lc = c;
                    asm volatile("" : "+s"(lh), "+v"(lc));
                    const int hk = lh;
                    if (A_AHEAD && gi + 1 < NG) {
                        asm volatile("" ::: "memory");
                        load_A(gi + 1);
                    } else if (k + 1 < HB) {  // wave-uniform: the first group of the next tile
                        asm volatile("" ::: "memory");
                        lh += HT;
                        load_A(0);
                    }
                    const int hyp0 = 16 * gi + 4 * g;
                    f2 ssum[4] = {splat(0.f), splat(0.f), splat(0.f), splat(0.f)};
#pragma unroll
                    for (int ch = 0; ch < CHW; ch++) {
                        f4 ev[4];
                        f2 sloc[4];
                        f2 pb = f2{(float)(sx0[ch] + 4 * c) - cx, sby[ch]};
                        asm volatile("" : "+v"(pb));
#pragma unroll
                        for (int m = 0; m < 4; m++) ppix[0][m] = f2{pb.x + (float)m, pb.y};
                        // the exact-z redo: arithmetic only
                        if (__builtin_expect(__any(hp_chunk_ex<false, SOFT, RSQ>(aex[gi], B8[ch], ppix[0], clampv, kA, kB, ev, sloc)), 0)) {
                            (void)hp_chunk_ex<true, SOFT>(aex[gi], B8[ch], ppix[0], clampv, kA, kB, ev, sloc);
                        }
                        if (SOFT) {
                            const f2 vf = splat(1.0f);
#pragma unroll
                            for (int r = 0; r < 4; r++) ssum[r] = pk_fma(sloc[r], vf, ssum[r]);
                        }
                        if constexpr (H16 != 0) {
                            store_rows_h16<H16, BF16, true>(reinterpret_cast<_Float16*>(err) + (size_t)(h0 + 16 * gi) * P, ev, P, p0[ch], g, c, true, 4);
                        } else if (ERR) {
                            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(err + (size_t)(h0 + 16 * gi) * P, 0, 0xffffffffu, 0x00020000);
                            const unsigned loff = ((unsigned)(4 * g) * (unsigned)P + (unsigned)p0[ch]) * 4u;
                            k2_stores_begin();
#pragma unroll
                            for (int r = 0; r < 4; r++) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, ev[r]), rsrc, loff, (unsigned)r * (unsigned)P * 4u, 2);
                            k2_stores_end();
                        }
                        if (ERR && !SOFT) {  // the pacing knobs of the error-images-only builds (k2_flags bits 16-23)
                            const int ps = (kflags >> 16) & 15, pn = (kflags >> 20) & 15;
                            for (int i = 0; i < ps; i++) __builtin_amdgcn_s_sleep(1);
                            for (int i = 0; i < pn; i++) asm volatile("s_nop 15");
                        }
                    }
                    if (SOFT) {
                        const float s0 = row16_sum(ssum[0].x + ssum[0].y), s1 = row16_sum(ssum[1].x + ssum[1].y);
                        const float s2 = row16_sum(ssum[2].x + ssum[2].y), s3 = row16_sum(ssum[3].x + ssum[3].y);
                        if (c == 0) {
                            float* dst = soft_part + (size_t)(pt * WAVES + wave) * N + hk + hyp0;
                            dst[0] = s0; dst[1] = s1; dst[2] = s2; dst[3] = s3;
                        }
                    }
                }
                if (k + 1 == HB) break;
                h0 += HT;
            }
            return;
        }
    }

    // The general path.  In the full-tile builds it runs once per tile of the walk (a partial last pixel tile, a far chunk, k2_flags bit 30), each further tile
    // starting like the first, with the operands of its first group; every other build has one tile and no way back up here
    [[maybe_unused]] int walked = 1;
[[maybe_unused]] next_tile:;
#pragma unroll
    for (int gi = 0; gi < NG; gi++) {
        if (16 * gi >= nh) break;
        if constexpr (FULL_TILE) {  // the walk: see lh, lc
            lh = h0; lc = c;
            asm volatile("" : "+s"(lh), "+v"(lc));
        }
        if (A_AHEAD && gi + 1 < NG) {
            asm volatile("" ::: "memory");  // keeps the compiler from hoisting the fetch to the top of the kernel (that is the up-front form)
            load_A(gi + 1);
        }
        const float nax = EX ? 0.f : -ax[EX ? 0 : gi], nay = EX ? 0.f : -ay[EX ? 0 : gi];  // x and y rows negated: the MFMA yields (-xc, -yc, zc)
        const int hyp0 = 16 * gi + 4 * g;
        // ANY: a group with a hypothesis whose split records clamp (k_pose_prep_split's mark in the translation quarter) takes the fp32 transform like a chunk of
        // far coordinates -- small maps are where P3P returns such poses (5 x 7 cells: 3 of 64 with |t_z| > 200 m).  The vector build is left as it was
        bool grp_far = false;
        if constexpr (ANY != 0 && EX) grp_far = __any((float)aex[gi].hx[3] != 0.f || (float)aex[gi].hy[3] != 0.f || (float)aex[gi].hz[3] != 0.f);
        f2 ssum[4] = {splat(0.f), splat(0.f), splat(0.f), splat(0.f)};
#pragma unroll
        for (int ch = 0; ch < CHW; ch++) {
            f4 ev[4];
            f2 sloc[4];
            if (G64) {
                f2 pb = f2{(float)(sx0[ch] + 4 * c) - cx, sby[ch]};  // the same numbers as a stored pair: (float)(column) - cx, (float)(row) - cy
                asm volatile("" : "+v"(pb));  // rebuilt per use: keeps the 8 position registers of a chunk from staying live across the whole kernel
#pragma unroll
                for (int m = 0; m < 4; m++) ppix[0][m] = f2{pb.x + (float)m, pb.y};
            }
            const f2 (&pp)[4] = ppix[G64 ? 0 : ch];
            if (EX) {
                if (__builtin_expect(oor[ch] || grp_far, 0)) {
                    // a coordinate beyond the split's range: this chunk through the fp32 transform (operands fetched here, the rare path)
                    const int hyp = min(16 * gi + c, nh - 1);
                    const float* rec = staged + (size_t)(h0 + hyp) * POSE_STRIDE + g;
                    float Bf[4];
#pragma unroll
                    for (int m = 0; m < 4; m++) Bf[m] = (g < 3) ? xyz[(size_t)min(p0[ch] + m, P - 1) * 3 + g] : 1.0f;
                    (void)hp_chunk<true, SOFT, false>(-rec[0], -rec[4], rec[8], Bf, pp, clampv, kA, kB, ev, sloc);
                } else if (__builtin_expect(__any(hp_chunk_ex<false, SOFT, RSQ>(aex[gi], B8[ch], pp, clampv, kA, kB, ev, sloc)), 0)) {
                    (void)hp_chunk_ex<true, SOFT>(aex[gi], B8[ch], pp, clampv, kA, kB, ev, sloc);
                }
            } else if (kflags & 2) {  // store schedule alone (measurement)
                ev[0] = ev[1] = ev[2] = ev[3] = f4{nax, nay, az[EX ? 0 : gi], (float)ch};
                sloc[0] = sloc[1] = sloc[2] = sloc[3] = splat(0.f);
            } else if (__builtin_expect(__any(hp_chunk<false, SOFT, LO>(nax, nay, az[EX ? 0 : gi], Bm[ch], pp, clampv, kA, kB, ev, sloc, &alo[LO ? gi : 0], B16[LO ? ch : 0])), 0)) {
                (void)hp_chunk<true, SOFT, LO>(nax, nay, az[EX ? 0 : gi], Bm[ch], pp, clampv, kA, kB, ev, sloc, &alo[LO ? gi : 0], B16[LO ? ch : 0]);
            }
            if constexpr (ANY == 2) {
                // per-cell validity of the sigmoids: exactly 1.0 on real cells, 0.0 on the cells that pad the last 4-cell group
                const int nv = P - p0[ch];
                if (SOFT) {
                    const f2 m01 = {nv > 0 ? 1.0f : 0.0f, nv > 1 ? 1.0f : 0.0f}, m23 = {nv > 2 ? 1.0f : 0.0f, nv > 3 ? 1.0f : 0.0f};
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        sloc[r] = pk_fma(soft_inlier2(f2{ev[r].x, ev[r].y}, kA, kB), m01, soft_inlier2(f2{ev[r].z, ev[r].w}, kA, kB) * m23);
                }
            }
            if (SOFT) {
                const f2 vf = splat(valid[ch] ? 1.0f : 0.0f);
#pragma unroll
                for (int r = 0; r < 4; r++) ssum[r] = pk_fma(sloc[r], vf, ssum[r]);
            }
            bool fast_stores = true;
            if constexpr (ANY != 0) {
                // the tail launch's lane stores its cells one by one
                fast_stores = ANY == 1;
                if (ERR && valid[ch] && !fast_stores) {
                    const int nv = P - p0[ch];
                    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(err + (size_t)(h0 + 16 * gi) * P, 0, 0xffffffffu, 0x00020000);
                    const unsigned loff = ((unsigned)(4 * g) * (unsigned)P + (unsigned)p0[ch]) * 4u;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if (hyp0 + r >= nh) continue;
                        const unsigned soff = (unsigned)r * (unsigned)P * 4u;
                        const float ex = ev[r].x, ey = ev[r].y, ez = ev[r].z, ew = ev[r].w;  // by value: a bit cast of a vector ELEMENT reads the vector's first dword
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ex), rsrc, loff, soff, 2);
                        if (nv > 1) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ey), rsrc, loff + 4u, soff, 2);
                        if (nv > 2) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ez), rsrc, loff + 8u, soff, 2);
                        if (nv > 3) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ew), rsrc, loff + 12u, soff, 2);
                    }
                }
            }
            if constexpr (H16 != 0) {
                if (valid[ch]) store_rows_h16<H16, BF16>(reinterpret_cast<_Float16*>(err) + (size_t)(h0 + 16 * gi) * P, ev, P, p0[ch], g, c, nh == HT, nh - hyp0);
            }
            if (H16 == 0 && ERR && valid[ch] && fast_stores) {
                // buffer store: the address is a wave-uniform row base in a scalar resource (the tile's first hypothesis of this group) + a scalar row offset +
                // a 32-bit lane offset (the lane's hypothesis quarter and pixel).  A global store's 64-bit vector address cost one vector instruction per store
                // (v_lshl_add_u64), 16 per 1 024 pairs of a kernel that is bound by vector issue; this form steps the rows on the scalar unit
                const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(err + (size_t)(h0 + 16 * gi) * P, 0, 0xffffffffu, 0x00020000);
                const unsigned loff = ((unsigned)(4 * g) * (unsigned)P + (unsigned)p0[ch]) * 4u;
                if (nh == HT) {
#pragma unroll
                    for (int r = 0; r < 4; r++) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, ev[r]), rsrc, loff, (unsigned)r * (unsigned)P * 4u, 2);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (hyp0 + r < nh) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, ev[r]), rsrc, loff, (unsigned)r * (unsigned)P * 4u, 2);
                }
            }
            if (ERR && !SOFT) {
                // error images only: the sigmoid arithmetic of the fused form is what spaces a wave's stores; without it the
                // wave idles for as long instead (k2_flags bits 16-19: units of 64 clocks per chunk, bits 20-23: units of 16) -- no VALU issue slots taken
                const int ps = (kflags >> 16) & 15, pn = (kflags >> 20) & 15;
                for (int i = 0; i < ps; i++) __builtin_amdgcn_s_sleep(1);
                for (int i = 0; i < pn; i++) asm volatile("s_nop 15");
            }
        }
        if (SOFT) {
            const float s0 = row16_sum(ssum[0].x + ssum[0].y), s1 = row16_sum(ssum[1].x + ssum[1].y);
            const float s2 = row16_sum(ssum[2].x + ssum[2].y), s3 = row16_sum(ssum[3].x + ssum[3].y);
            if (c == 0) {
                float* dst = !PW ? s_soft + wave * HT + hyp0 : soft_part + (size_t)(pt * WAVES + wave) * N + (FULL_TILE ? lh : h0) + hyp0;
                if (hyp0 + 0 < nh) dst[0] = s0;
                if (hyp0 + 1 < nh) dst[1] = s1;
                if (hyp0 + 2 < nh) dst[2] = s2;
                if (hyp0 + 3 < nh) dst[3] = s3;
            }
        }
    }
    if constexpr (FULL_TILE) {
        static_assert(A_AHEAD, "a further tile starts with the operands of its first group alone");
        if (walked < HB) {
            walked++;
            h0 += HT;
            nh = min(HT, N - h0);
            lh = h0;
            load_A(0);
            goto next_tile;
        }
    }
    if (SOFT && !PW) {
        __syncthreads();
        if (tid < nh) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; w++) s += s_soft[w * HT + tid];
            soft_part[(size_t)pt * N + h0 + tid] = s;
        }
    }
}

// --------------------------------------------------------------------------------------------------
// K2, persistent pipelined form (round 3).  Small tiles (NG x 16 hypotheses x one 64-pixel chunk per wave) stream their stores best, but as
// short-lived workgroups each of them starts with global loads that queue BEHIND the stores of the other waves of its CU in the CU's
// in-order memory pipe, and a store-bound kernel keeps that pipe full (k2_lab: small tiles 774 us store-only, 846 arithmetic-only, 981
// together).  Here the waves are persistent and software-pipelined: the operands of tile i + 2 (4 coordinate dwords + 3 NG pose dwords per
// lane) are requested BEFORE the stores of tile i are issued, so -- the memory counter of a wave retires in order -- waiting for the operands
// of tile i + 1 never waits for a store, and no wave ever waits for its stores at all until the kernel ends.  The tile sequence of the grid
// follows the order the dispatcher would give short-lived workgroups: pixel units (4 adjacent chunks = the 4 waves of a workgroup) innermost,
// XCD x owning the units u % 8 == x.
// --------------------------------------------------------------------------------------------------
template <int NG>
struct K2Ops {
    float B[4];
    float A[NG][3];
};

template <int NG, int WAVES, bool ERR, bool SOFT, bool UV>
__global__ __launch_bounds__(WAVES * 64) void k_reproject_ps(const float* __restrict__ staged, const float* __restrict__ xyz,
                                                             const float* __restrict__ uv, float* __restrict__ err,
                                                             float* __restrict__ soft_part, int N, int P, int W, float cx, float cy,
                                                             float clampv, float kA, float kB, int kflags, int Nf, long long xyz_stride,
                                                             long long uv_stride) {
    constexpr int HT = 16 * NG;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int xcd = blockIdx.x & 7, lwg = blockIdx.x >> 3, GX = gridDim.x >> 3;  // gridDim.x is a multiple of 8
    const int CR = (P + 63) >> 6;                   // 64-pixel chunks per row
    const int UR = (CR + WAVES - 1) / WAVES;        // pixel units (WAVES adjacent chunks) per row
    const int URX = (UR + 7) >> 3;                  // ... per XCD
    const int NRG = (N + HT - 1) / HT;              // hypothesis groups
    const int TT = NRG * URX;                       // tiles of this XCD's workgroup sequence

    // tile tw of this workgroup -> (first hypothesis, chunk of this wave); chunk < 0: nothing to do
    auto decode = [&](int tw, int& h0, int& chunk) {
        const int rg = tw / URX, ux = tw - rg * URX;
        const int unit = ux * 8 + xcd;
        h0 = rg * HT;
        chunk = (tw < TT && unit < UR) ? unit * WAVES + wave : -1;
        if (chunk >= CR) chunk = -1;
    };
    // the loads of a tile are issued unconditionally (a tile beyond the end re-reads the last one's operands): the number of memory
    // operations between a tile's loads and their first use is then the same on every path, and the wait in front of that use is never vmcnt(0)
    auto issue = [&](int tw, K2Ops<NG>& o) {
        int h0, chunk;
        decode(min(tw, TT - 1), h0, chunk);
        chunk = max(chunk, 0);
        const int nh = min(HT, N - h0);
        const float* fx = xyz + (long long)(h0 / Nf) * xyz_stride;
        const int p0 = chunk * 64 + 4 * c;
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int pc = min(p0 + m, P - 1);
            o.B[m] = fx[(size_t)pc * 3 + min(g, 2)];
        }
#pragma unroll
        for (int gi = 0; gi < NG; gi++) {
            const int hyp = min(16 * gi + c, nh - 1);
            const float* rec = staged + (size_t)(h0 + hyp) * POSE_STRIDE + g;
            o.A[gi][0] = rec[0]; o.A[gi][1] = rec[4]; o.A[gi][2] = rec[8];
        }
    };
    auto compute = [&](int tw, const K2Ops<NG>& o) {
        int h0, chunk;
        decode(tw, h0, chunk);
        if (chunk < 0) return;
        const int nh = min(HT, N - h0);
        const int p0 = chunk * 64 + 4 * c;
        const bool valid = p0 < P;
        const float Bv[4] = {g < 3 ? o.B[0] : 1.0f, g < 3 ? o.B[1] : 1.0f, g < 3 ? o.B[2] : 1.0f, g < 3 ? o.B[3] : 1.0f};  // the k = 3 row of B is 1
        f2 ppix[4];
        if (UV) {
            const float* fu = uv + (long long)(h0 / Nf) * uv_stride;
            if (valid) {
                const f4* su = reinterpret_cast<const f4*>(fu + (size_t)p0 * 2);
                const f4 u0 = su[0], u1 = su[1];
                ppix[0] = f2{u0.x - cx, u0.y - cy}; ppix[1] = f2{u0.z - cx, u0.w - cy};
                ppix[2] = f2{u1.x - cx, u1.y - cy}; ppix[3] = f2{u1.z - cx, u1.w - cy};
            } else {
                ppix[0] = ppix[1] = ppix[2] = ppix[3] = splat(0.f);
            }
        } else if ((W & 63) == 0) {
            const int cpr = W >> 6;
            const int y = chunk / cpr, xc0 = (chunk - y * cpr) * 64;
            const float fy_ = (float)y - cy, fx_ = (float)(xc0 + 4 * c) - cx;
#pragma unroll
            for (int m = 0; m < 4; m++) ppix[m] = f2{fx_ + (float)m, fy_};
        } else {
            int y = p0 / W, x = p0 - y * W;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                ppix[m] = f2{(float)x - cx, (float)y - cy};
                if (++x == W) { x = 0; y++; }
            }
        }
#pragma unroll
        for (int gi = 0; gi < NG; gi++) {
            if (16 * gi >= nh) break;
            const float nax = -o.A[gi][0], nay = -o.A[gi][1], az = o.A[gi][2];
            const int hyp0 = 16 * gi + 4 * g;
            f4 ev[4];
            f2 sloc[4];
            if (kflags & 2) {
                ev[0] = ev[1] = ev[2] = ev[3] = f4{nax, nay, az, Bv[0]};
                sloc[0] = sloc[1] = sloc[2] = sloc[3] = splat(0.f);
            } else if (__builtin_expect(__any(hp_chunk<false, SOFT>(nax, nay, az, Bv, ppix, clampv, kA, kB, ev, sloc)), 0)) {
                (void)hp_chunk<true, SOFT>(nax, nay, az, Bv, ppix, clampv, kA, kB, ev, sloc);
            }
            if (ERR && valid) {
                f4* dst = reinterpret_cast<f4*>(err + (size_t)(h0 + hyp0) * P + p0);
                const size_t rs = (size_t)P / 4;
                if (nh == HT) {
#pragma unroll
                    for (int r = 0; r < 4; r++) __builtin_nontemporal_store(ev[r], dst + r * rs);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (hyp0 + r < nh) __builtin_nontemporal_store(ev[r], dst + r * rs);
                }
            }
            if (SOFT) {
                const float vf = valid ? 1.0f : 0.0f;
                const float s0 = row16_sum((sloc[0].x + sloc[0].y) * vf), s1 = row16_sum((sloc[1].x + sloc[1].y) * vf);
                const float s2 = row16_sum((sloc[2].x + sloc[2].y) * vf), s3 = row16_sum((sloc[3].x + sloc[3].y) * vf);
                if (c == 0) {  // one partial row per 64-pixel chunk
                    float* dst = soft_part + (size_t)chunk * N + h0 + hyp0;
                    if (nh == HT) {
                        __builtin_nontemporal_store(f4{s0, s1, s2, s3}, reinterpret_cast<f4*>(dst));
                    } else {
                        if (hyp0 + 0 < nh) dst[0] = s0;
                        if (hyp0 + 1 < nh) dst[1] = s1;
                        if (hyp0 + 2 < nh) dst[2] = s2;
                        if (hyp0 + 3 < nh) dst[3] = s3;
                    }
                }
            }
        }
    };

    // three operand sets in rotation (unrolled by hand: a register copy of a set whose loads are still in flight would have to wait for them)
    K2Ops<NG> o0, o1, o2;
    issue(lwg, o0);
    issue(lwg + GX, o1);
    for (int tw = lwg; tw < TT; tw += 3 * GX) {
        issue(tw + 2 * GX, o2);
        compute(tw, o0);
        issue(tw + 3 * GX, o0);
        compute(tw + GX, o1);
        issue(tw + 4 * GX, o1);
        compute(tw + 2 * GX, o2);
    }
}

template <int NG, int WAVES>
static hipError_t launch_reproject_ps(hipStream_t st, int N, const float* staged, const FrameDev& F, float clampv, float* err, float kA, float kB,
                                      float* soft_part, int Nf, int kflags, hipEvent_t evA, hipEvent_t evB) {
    // (the partial sums leave as 16-byte stores: the plan has refused N % 4 != 0 with them)
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    int per_cu = (kflags >> 8) & 0xff;  // k2_flags bits 8..15: persistent workgroups per CU (0 = default)
    if (per_cu <= 0) per_cu = 3;
    const int grid = ((cus * per_cu + 7) / 8) * 8;
    const bool ERR = err != nullptr, SOFT = soft_part != nullptr, UV = F.uv != nullptr;
#define DSAC_K2P(E, S, U)                                                                                                               \
    hipExtLaunchKernelGGL((k_reproject_ps<NG, WAVES, E, S, U>), dim3(grid), dim3(WAVES * 64), 0, st, evA, evB, 0, staged, F.xyz, F.uv, err,   \
                          soft_part, N, F.P, F.W, F.cx, F.cy, clampv, kA, kB, kflags, Nf, F.xyz_stride, F.uv_stride)
    if (ERR && SOFT) { if (UV) DSAC_K2P(true, true, true); else DSAC_K2P(true, true, false); }
    else if (ERR) { if (UV) DSAC_K2P(true, false, true); else DSAC_K2P(true, false, false); }
    else if (SOFT) { if (UV) DSAC_K2P(false, true, true); else DSAC_K2P(false, true, false); }
#undef DSAC_K2P
    return hipGetLastError();
}

// The store layout of a bfloat16 build (EX = 5: 8-byte stores, 6: 16-byte stores after the lane exchange) for one instantiation.  Two builds of the small tile
// at its 168-register budget (implicit grid, W % 64 != 0) spill 12 bytes per lane in one layout and nothing in the other -- error images only in layout 1, err + soft
// in layout 2, as their binary16 twins do --; the bfloat16 call takes the other layout there, whatever "k2_f16_store" says: the stored values do not depend on
// the layout, and no bfloat16 build needs scratch.  Every other EX is returned as it is (the float and binary16 kernels keep their instantiations)
template <int NG, int CHW, int MINW, int EX>
constexpr int k2_bf16_exf(bool soft, bool uv, bool g64) {
    if (EX >= 5 && NG == 4 && CHW == 1 && MINW == 3 && !uv && !g64) return soft ? 5 : 6;
    return EX;
}
template <int NG, int CHW, int WAVES, bool PW, int MINW = 1, bool LO = false, int EX = 0, int ANY = 0>
static hipError_t launch_reproject_st(hipStream_t st, int N, const float* staged, const FrameDev& F, float clampv, float* err, float kA, float kB,
                                      float* soft_part, int Nf, int kflags, hipEvent_t evA, hipEvent_t evB, const float* staged_lo = nullptr,
                                      const void* split = nullptr) {
    const int tile = WAVES * CHW * 64;
    static_assert(PW || WAVES > 1, "one-wave workgroups write per-wave partial sums");
    const int PT = (F.P + tile - 1) / tile;
    // hypothesis walks (the plan's hyp_walk, in the kernel's flag bits 6-7): a workgroup scores that many tiles; the plan has made sure they divide the tiles
    const int NTa = k2_walks(N, NG, 1 << ((kflags >> K2_KFLAG_WALK_SHIFT) & 3));
    const int grid = (kflags & 32) ? PT * NTa : WAVES == 1 ? ((PT + 31) / 32) * 32 * NTa : ((PT + 7) / 8) * 8 * NTa;
    const bool ERR = err != nullptr, SOFT = soft_part != nullptr, UV = F.uv != nullptr;
    const bool G64 = !UV && (F.W & 63) == 0;
#define DSAC_K2S(E, S, U, G)                                                                                                               \
    hipExtLaunchKernelGGL((k_reproject_st<NG, CHW, WAVES, PW, E, S, U, G, MINW, LO, k2_bf16_exf<NG, CHW, MINW, EX>(S, U, G), ANY>), dim3(grid), dim3(WAVES * 64), 0, st, evA, evB, 0, staged, F.xyz, F.uv, err, \
                          soft_part, N, F.P, F.W, PT, F.cx, F.cy, clampv, kA, kB, kflags, Nf, F.xyz_stride, F.uv_stride, staged_lo, split, F.cams)
    if (ERR && SOFT) { if (UV) DSAC_K2S(true, true, true, false); else if (G64) DSAC_K2S(true, true, false, true); else DSAC_K2S(true, true, false, false); }
    else if (ERR) { if (UV) DSAC_K2S(true, false, true, false); else if (G64) DSAC_K2S(true, false, false, true); else DSAC_K2S(true, false, false, false); }
    else if (SOFT) {
        if constexpr (EX >= 3) return hipErrorInvalidValue;  // the half-store builds exist with an error image only
        else { if (UV) DSAC_K2S(false, true, true, false); else if (G64) DSAC_K2S(false, true, false, true); else DSAC_K2S(false, true, false, false); }
    }
#undef DSAC_K2S
    return hipGetLastError();
}

// The any-map build of the exact form: the main launch (ANY = 1) on the tile <16 NG hypotheses, 64 CHW cells>, then -- only when the cell count is no multiple
// of 4 -- the tail launch (ANY = 2) for the lane of the last 1-3 cells, whose sums go to one more partial row.  A timing pair spans both launches.
template <int NG, int CHW, int MINW>
static hipError_t launch_reproject_any(hipStream_t st, int N, const float* staged, const FrameDev& F, float clampv, float* err, float kA, float kB, float* soft_part,
                                       int Nf, int kflags, hipEvent_t evA, hipEvent_t evB, const void* split) {
    const bool tail = (F.P & 3) != 0;
    const int rows = (F.P + CHW * 64 - 1) / (CHW * 64);  // the main launch's partial rows; the tail's is the plan's one more
    hipError_t e = launch_reproject_st<NG, CHW, 1, true, MINW, false, 2, 1>(st, N, staged, F, clampv, err, kA, kB, soft_part, Nf, kflags, evA, tail ? nullptr : evB, nullptr, split);
    if (e != hipSuccess || !tail) return e;
    const int NTa = (N + 63) / 64;
    float* part = soft_part ? soft_part + (size_t)rows * N : nullptr;  // row `rows` <= ceil(P / 64) < reproject_num_pixel_tiles(P)
    const bool ERR = err != nullptr, SOFT = soft_part != nullptr, UV = F.uv != nullptr;
#define DSAC_K2T(E, S, U)                                                                                                                              \
    hipExtLaunchKernelGGL((k_reproject_st<4, 1, 1, true, E, S, U, false, 3, false, 2, 2>), dim3(NTa), dim3(64), 0, st, nullptr, evB, 0, staged, F.xyz, F.uv, err, part, N, \
                          F.P, F.W, 1, F.cx, F.cy, clampv, kA, kB, kflags | 32, Nf, F.xyz_stride, F.uv_stride, nullptr, split, F.cams)
    if (ERR && SOFT) { if (UV) DSAC_K2T(true, true, true); else DSAC_K2T(true, true, false); }
    else if (ERR) { if (UV) DSAC_K2T(true, false, true); else DSAC_K2T(true, false, false); }
    else if (SOFT) { if (UV) DSAC_K2T(false, true, true); else DSAC_K2T(false, true, false); }
#undef DSAC_K2T
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------
// K2, PRECISE form (round 5; dsac_set_option("k2_flags", bit 25)).  The reference projects in double (core/cnn_softam.h:319-362: cv::projectPoints of a
// float point under a double pose) and rounds the residual to float at the end; the fast forms above carry fp32 records into an fp32 matrix-core
// transform, whose four roundings at the magnitude of the partial sums (f * R.X ~ 1e6, z ~ 3e3) are what the suite measures as up to 5.9e-4 px on cells
// close to the camera plane (profiles/r04_final2_parity_margins.txt) -- inside the stated 1e-3, but with a margin of 1.7x, and with a softmax weight in
// a tie of two unrelated hypotheses moving by an estimated 2.3e-4 (stated: 1e-4).  This form evaluates the reference's own arithmetic: the pose records
// in fp64 (Rodrigues of the cv pose in the workgroup's prologue, intrinsics folded in -- no staged fp32 record at all), the rigid transform as three
// chains of three v_fma_f64 per (hypothesis, cell) -- fp64 FMA issues at the rate of an unpacked fp32 FMA on this chip --, the perspective division in
// fp64 through one Newton step on v_rcp_f32's seed, and ONE rounding to float of each image-plane difference; only |d| = sqrt(du^2 + dv^2), the clamp and
// the sigmoid stay in fp32.  Measured residual error against the oracle: see profiles/r05_k2_precise_ab.txt.  Cost: 27 % more issue cycles per pair than
// the matrix-core form (priced), hidden only in part by the store schedule -- a parity mode, not the default.
// Layout: the VALU form's (lane = 4 consecutive cells, hypothesis loop over an LDS tile of records; a wave store is 1 KiB of one error-image row).
// --------------------------------------------------------------------------------------------------
DM_INLINE f2 soft_inlier2_hl(f2 e, float kA, float kAl, float kB, float kBl) {
    const f2 t = pk_fma(splat(kA), e, splat(kB)) + pk_fma(splat(kAl), e, splat(kBl));
    f2 ex;
    ex.x = __builtin_amdgcn_exp2f(t.x);
    ex.y = __builtin_amdgcn_exp2f(t.y);
    const f2 d = ex + splat(1.0f);
    f2 r;
    r.x = __builtin_amdgcn_rcpf(d.x);
    r.y = __builtin_amdgcn_rcpf(d.y);
    return pk_fma(pk_fma(-d, r, splat(1.0f)), r, r);
}

template <int HT, bool ERR, bool SOFT, bool UV, bool DIAG>
__global__ __launch_bounds__(K2_THREADS) void k_reproject_prec(const double* __restrict__ poses, const float* __restrict__ xyz, const float* __restrict__ uv,
                                                               float* __restrict__ err, float* __restrict__ soft_part, int N, int P, int W, int PT,
                                                               float fx, float fy, float cx, float cy, float clampv, float kA, float kB, int Nf,
                                                               long long xyz_stride, long long uv_stride, float kAl, float kBl, int rec32, int diag_arg) {
    const int diag = DIAG ? diag_arg : 0;  // the diagnostic switches only exist in the DIAG instantiation: the parity mode itself pays nothing for them
    const int b = blockIdx.x;
    const int q = b >> 3, PTG = (PT + 7) >> 3;
    const int ht = q / PTG, pt = (q % PTG) * 8 + (b & 7);  // XCD-aware, pixel tiles innermost
    if (pt >= PT) return;
    const int h0 = ht * HT;
    const int nh = min(HT, N - h0);
    const int tid = threadIdx.x;
    {
        const int frame = h0 / Nf;
        xyz += (long long)frame * xyz_stride;
        if (UV) uv += (long long)frame * uv_stride;
    }
    __shared__ __attribute__((aligned(16))) double s_rec[HT * 12];
    __shared__ double s_red[SOFT ? (K2_THREADS / 64) * HT : 1];
    if (tid < nh) {  // record of hypothesis h0 + tid: [fx R0 | fx t0 ; fy R1 | fy t1 ; R2 | t2] in double
        const double* ps = poses + (size_t)(h0 + tid) * 6;
        double r[3] = {ps[0], ps[1], ps[2]}, R[9];
        dm::rodrigues_v2m<false>(r, R, nullptr);
        double* o = s_rec + tid * 12;
        const double dfx = fx, dfy = fy;
        o[0] = dfx * R[0]; o[1] = dfx * R[1]; o[2] = dfx * R[2]; o[3] = dfx * ps[3];
        o[4] = dfy * R[3]; o[5] = dfy * R[4]; o[6] = dfy * R[5]; o[7] = dfy * ps[4];
        o[8] = R[6]; o[9] = R[7]; o[10] = R[8]; o[11] = ps[5];
        // diagnostic (k2_flags bit 26): the records rounded to float as the fast forms stage them, everything else exact -- isolates what the fp32 RECORD alone
        // costs (tests/test_gpu_k2_precise.py: it is the bulk of the fast form's score error, a systematic shift of all of a hypothesis' projections)
        if (rec32) {
#pragma unroll
            for (int k = 0; k < 12; k++) o[k] = (double)(float)o[k];
        }
    }
    const int p0 = (pt * K2_THREADS + tid) * 4;
    const bool valid = p0 < P;  // P % 4 == 0
    double X[4], Y[4], Z[4], pu[4], pv[4];
    if (valid) {
        const f4* src = reinterpret_cast<const f4*>(xyz + (size_t)p0 * 3);
        const f4 a = src[0], bb = src[1], c = src[2];
        X[0] = a.x; Y[0] = a.y; Z[0] = a.z;
        X[1] = a.w; Y[1] = bb.x; Z[1] = bb.y;
        X[2] = bb.z; Y[2] = bb.w; Z[2] = c.x;
        X[3] = c.y; Y[3] = c.z; Z[3] = c.w;
        if (UV) {
            const f4* su = reinterpret_cast<const f4*>(uv + (size_t)p0 * 2);
            const f4 u0 = su[0], u1 = su[1];
            pu[0] = (double)u0.x - (double)cx; pv[0] = (double)u0.y - (double)cy; pu[1] = (double)u0.z - (double)cx; pv[1] = (double)u0.w - (double)cy;
            pu[2] = (double)u1.x - (double)cx; pv[2] = (double)u1.y - (double)cy; pu[3] = (double)u1.z - (double)cx; pv[3] = (double)u1.w - (double)cy;
        } else {
            const int y = p0 / W, x = p0 - y * W;  // 4 | W for the implicit grid of this form: the four cells share a row
#pragma unroll
            for (int k = 0; k < 4; k++) { pu[k] = (double)(x + k) - (double)cx; pv[k] = (double)y - (double)cy; }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) { X[k] = Y[k] = 0.0; Z[k] = 1.0; pu[k] = pv[k] = 0.0; }
    }
    __syncthreads();
    float* erow = ERR ? err + (size_t)h0 * P + p0 : nullptr;
    const int wave = tid >> 6, lane = tid & 63;
    for (int h = 0; h < nh; h++) {
        const double* sp = s_rec + h * 12;
        const double a0 = sp[0], a1 = sp[1], a2 = sp[2], a3 = sp[3], b0 = sp[4], b1 = sp[5], b2 = sp[6], b3 = sp[7], c0 = sp[8], c1 = sp[9], c2 = sp[10], c3 = sp[11];
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double xc = fma(a0, X[k], fma(a1, Y[k], fma(a2, Z[k], a3)));
            const double yc = fma(b0, X[k], fma(b1, Y[k], fma(b2, Z[k], b3)));
            const double zc = fma(c0, X[k], fma(c1, Y[k], fma(c2, Z[k], c3)));
            // 1 / zc in double: v_rcp_f32's seed (1 ulp, 2^-23) and one Newton step (2^-46: a relative 1.4e-14, i.e. 6e-12 px at the image border -- far
            // below the float the difference is rounded to); projectPoints: z = Z ? 1/Z : 1
            float du, dv;
            if (diag & 4) {
                // diagnostic (k2_diag bit 2, round 6): the exact camera-frame point rounded ONCE to float, then the fast forms' fp32 tail -- what a form
                // with an exact transform in front of hp_chunk's arithmetic would compute (bit 3: one Newton step on v_rcp_f32's result)
                const float xf = (float)xc, yf = (float)yc, zf = (float)zc;
                float izf = __builtin_amdgcn_rcpf(zf);
                if (diag & 8) izf = fmaf(fmaf(-zf, izf, 1.0f), izf, izf);
                izf = (zf == 0.0f) ? 1.0f : izf;
                du = fmaf(-xf, izf, (float)pu[k]);
                dv = fmaf(-yf, izf, (float)pv[k]);
            } else {
                double xq = xc, yq = yc, zq = zc;
                if (diag & 2) { xq = (double)(float)xc; yq = (double)(float)yc; zq = (double)(float)zc; }  // bit 1: the point rounded to float, the tail exact
                double iz = (double)__builtin_amdgcn_rcpf((float)zq);
                iz = fma(fma(-zq, iz, 1.0), iz, iz);
                iz = (zq == 0.0) ? 1.0 : iz;
                du = (float)fma(-xq, iz, pu[k]);  // cell position minus projection: one rounding to float, like the reference's Point2f difference
                dv = (float)fma(-yq, iz, pv[k]);
            }
            e[k] = fminf(__builtin_amdgcn_sqrtf(fmaf(dv, dv, du * du)), clampv);
        }
        if (ERR && valid) __builtin_nontemporal_store(f4{e[0], e[1], e[2], e[3]}, reinterpret_cast<f4*>(erow + (size_t)h * P));
        if (SOFT) {
            // the sums in double from the lane's four sigmoids on: an fp32 tile sum (<= 1024) is rounded to 6e-5, and 300 such tiles put ~1e-3 on a score of
            // ~2e4 -- 2e-4 on a softmax weight in a tie, twice the stated 1e-4
            // ... and the sigmoid without the systematic part of its fp32 error: the exponent from (high, low) pairs of the two constants (a rounded kA / kB shifts
            // every cell's exponent the same way: ~1e-3 on a score), the reciprocal polished by one Newton step
            // k2_diag bit 4: the sigmoid's constants as single floats; bit 5: its reciprocal unpolished; bit 6: the wave's sum in fp32 (the fast forms' sums)
            const float kAl_ = (diag & 16) ? 0.f : kAl, kBl_ = (diag & 16) ? 0.f : kBl;
            f2 s2;
            if (diag & 32) s2 = soft_inlier2(f2{e[0], e[1]}, kA, kB) + soft_inlier2(f2{e[2], e[3]}, kA, kB);
            else s2 = soft_inlier2_hl(f2{e[0], e[1]}, kA, kAl_, kB, kBl_) + soft_inlier2_hl(f2{e[2], e[3]}, kA, kAl_, kB, kBl_);
            double s;
            if (diag & 64) {
                float sf = valid ? s2.x + s2.y : 0.f;
                sf = wave_sum(sf);
                s = (double)sf;
            } else {
                s = valid ? (double)s2.x + (double)s2.y : 0.0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            }
            if (lane == 0) s_red[wave * HT + h] = s;
        }
    }
    if (SOFT) {
        __syncthreads();
        if (tid < nh) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < K2_THREADS / 64; w++) s += s_red[w * HT + tid];
            // the partial rows are floats: the tile's sum travels as a (high, low) pair of rows, which the fp64 reduction adds back together
            const float hi = (float)s;
            soft_part[(size_t)pt * N + h0 + tid] = hi;
            soft_part[(size_t)(PT + pt) * N + h0 + tid] = (float)(s - (double)hi);
        }
    }
}

template <int HT>
static hipError_t launch_reproject_prec(hipStream_t st, int N, const double* poses, const FrameDev& F, float clampv, float* err, double kAd, double kBd,
                                        float* soft_part, int Nf, hipEvent_t evA, hipEvent_t evB, int rec32, int diag) {
    const float kA = (float)kAd, kB = (float)kBd, kAl = (float)(kAd - (double)kA), kBl = (float)(kBd - (double)kB);
    const int PT = (F.P + K2_THREADS * 4 - 1) / (K2_THREADS * 4);
    const int NTa = (N + HT - 1) / HT;
    const int grid = ((PT + 7) / 8) * 8 * NTa;
    const bool ERR = err != nullptr, SOFT = soft_part != nullptr, UV = F.uv != nullptr;
#define DSAC_K2P(E, S, U)                                                                                                                       \
    do { if (diag) hipExtLaunchKernelGGL((k_reproject_prec<HT, E, S, U, true>), dim3(grid), dim3(K2_THREADS), 0, st, evA, evB, 0, poses, F.xyz, F.uv, err, soft_part, N, F.P, \
                          F.W, PT, F.fx, F.fy, F.cx, F.cy, clampv, kA, kB, Nf, F.xyz_stride, F.uv_stride, kAl, kBl, rec32, diag); \
         else hipExtLaunchKernelGGL((k_reproject_prec<HT, E, S, U, false>), dim3(grid), dim3(K2_THREADS), 0, st, evA, evB, 0, poses, F.xyz, F.uv, err, soft_part, N, F.P, \
                          F.W, PT, F.fx, F.fy, F.cx, F.cy, clampv, kA, kB, Nf, F.xyz_stride, F.uv_stride, kAl, kBl, rec32, 0); } while (0)
    if (ERR && SOFT) { if (UV) DSAC_K2P(true, true, true); else DSAC_K2P(true, true, false); }
    else if (ERR) { if (UV) DSAC_K2P(true, false, true); else DSAC_K2P(true, false, false); }
    else if (SOFT) { if (UV) DSAC_K2P(false, true, true); else DSAC_K2P(false, true, false); }
#undef DSAC_K2P
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------
// The two degradations of the exact form made countable (dsac_k2_range_census; not in any hot path).  Wave w of the grid looks at 64-cell chunk w of the
// frame batch exactly as k_reproject_st does (cells beyond the map repeat the last one; split_B's own predicate); thread t < N splits the records of
// hypothesis t as k_pose_prep_split does and notes a clamped piece or a non-finite entry.
// --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_k2_census(int N, const double* __restrict__ poses, float fx, float fy, int ex, const float* __restrict__ xyz, int P, int frames,
                                                   long long xyz_stride, unsigned long long* __restrict__ out, const float4* __restrict__ cams, int Nf) {
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int CR = (P + 63) >> 6;
    const int w = t >> 6;  // wave-uniform
    if (w < frames * CR) {
        const int f = w / CR, chunk = w - f * CR;
        const float* src = xyz + (long long)f * xyz_stride + (size_t)min(chunk * 64 + lane, P - 1) * 3;
        bool o = false;
#pragma unroll
        for (int k = 0; k < 3; k++) (void)split_B(src[k], o);
        if (__any(o) && lane == 0) atomicAdd(out, 1ull);
    }
    if (t < N) {
        if (cams) {  // as k_pose_prep_split: the focal lengths and the exponent of the hypothesis' own frame
            pose_focal(cams, t, Nf, fx, fy);
            ex = split_exponent_of(fx, fy);
        }
        double rv[3] = {poses[6 * t], poses[6 * t + 1], poses[6 * t + 2]};
        double R[9];
        dm::rodrigues_v2m<false>(rv, R, nullptr);
        bool bad = false;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double f = r == 0 ? -(double)fx : r == 1 ? -(double)fy : 1.0;
            const int E = r < 2 ? ex : 0;
            const double a[4] = {f * R[3 * r], f * R[3 * r + 1], f * R[3 * r + 2], f * poses[6 * t + 3 + r]};
            bad |= split_row_bad(a, E);
        }
        if (bad) atomicAdd(out + 1, 1ull);
    }
}
hipError_t k2_range_census(hipStream_t st, int N, const double* poses, const FrameDev& F, unsigned long long* out2, int Nf) {
    const int frames = F.frames > 1 ? F.frames : 1;
    const long long waves = (long long)frames * ((F.P + 63) / 64);
    const long long threads = waves * 64 > N ? waves * 64 : N;
    if (threads <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_k2_census, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, N, poses, F.fx, F.fy, pose_split_exponent(F), F.xyz, F.P, frames, F.xyz_stride, out2, F.cams, Nf);
    return hipGetLastError();
}

template <int PX, int HT, bool SPOSE>
static hipError_t launch_reproject(hipStream_t st, int N, const float* staged, const FrameDev& F, float clampv, float* err, float kA, float kB,
                                   float* soft_part, int Nf, bool pixel_minor, int kflags, hipEvent_t evA, hipEvent_t evB) {
    const int tile = K2_THREADS * PX;
    const int PT = (F.P + tile - 1) / tile;
    const int NTa = (N + HT - 1) / HT;
    const int grid = ((PT + 7) / 8) * 8 * NTa;
    const int NT = pixel_minor ? -NTa : NTa;
    const bool ERR = err != nullptr, SOFT = soft_part != nullptr, UV = F.uv != nullptr;
#define DSAC_K2(E, S, U)                                                                                                              \
    hipExtLaunchKernelGGL((k_reproject<PX, HT, E, S, U, SPOSE>), dim3(grid), dim3(K2_THREADS), 0, st, evA, evB, 0, staged, F.xyz, F.uv, err, soft_part, \
                          N, F.P, F.W, PT, NT, F.cx, F.cy, clampv, kA, kB, kflags, Nf, F.xyz_stride, F.uv_stride)
    if (ERR && SOFT) { if (UV) DSAC_K2(true, true, true); else DSAC_K2(true, true, false); }
    else if (ERR) { if (UV) DSAC_K2(true, false, true); else DSAC_K2(true, false, false); }
    else if (SOFT) { if (UV) DSAC_K2(false, true, true); else DSAC_K2(false, true, false); }
#undef DSAC_K2
    return hipGetLastError();
}

// K2: enqueue the kernel of a plan (k2_plan.h).  Every decision -- form, kernel, block order, flags -- is the plan's; the switches below only turn its tile
// numbers into template arguments, through the id lists the plan resolved them from.
static_assert(K2_WG == K2_THREADS, "k2_plan.h counts partial-sum rows with the workgroup size of the kernels");
static_assert(K2_STATUS_OK == (int)hipSuccess && K2_STATUS_INVALID == (int)hipErrorInvalidValue && K2_STATUS_NOT_SUPPORTED == (int)hipErrorNotSupported,
              "k2_plan.h spells the HIP status values out");
hipError_t reproject(hipStream_t st, const K2Plan& plan, int N, const float* staged, const FrameDev& F, float clampv, float* err, float tau, float beta,
                     float* soft_part, const K2Call& call) {
    if (plan.status != K2_STATUS_OK) return (hipError_t)plan.status;
    const K2Kernel& k = plan.k;
    const float LOG2E = 1.4426950408889634f;
    const float kA = beta * LOG2E, kB = -beta * tau * LOG2E;
    // the kernels take the plan's hypothesis walk in flag bits 6-7 (log2); whatever "k2_flags" held there is dropped
    const int Nf = plan.Nf, kf = (plan.kflags & ~(3 << K2_KFLAG_WALK_SHIFT)) | ((plan.hyp_walk == 4 ? 2 : plan.hyp_walk == 2 ? 1 : 0) << K2_KFLAG_WALK_SHIFT);
    const bool pm = plan.pixel_minor;
    // timing events (dsac_profile_enable): attached to the kernel's own dispatch (hipExtLaunchKernelGGL) instead of two event records on the
    // stream, which cost ~7 us of bubble each (one 640x480 frame: 100 us per step with them, 86 without)
    hipEvent_t evA = call.ev_start, evB = call.ev_stop;
#define DSAC_VA(PX_, HT_, SP_) launch_reproject<PX_, HT_, SP_>(st, N, staged, F, clampv, err, kA, kB, soft_part, Nf, pm, kf, evA, evB)
#define DSAC_HP(HT_, CH_) launch_reproject_hp<HT_, CH_>(st, N, staged, F, clampv, err, kA, kB, soft_part, Nf, pm, kf, evA, evB)
#define DSAC_ST(NG_, CH_, WV_, PW_, MW_) launch_reproject_st<NG_, CH_, WV_, PW_, MW_>(st, N, staged, F, clampv, err, kA, kB, soft_part, Nf, kf, evA, evB)
#define DSAC_PS(NG_) launch_reproject_ps<NG_, 4>(st, N, staged, F, clampv, err, kA, kB, soft_part, Nf, kf, evA, evB)
#define DSAC_LO(NG_, CH_, MW_) launch_reproject_st<NG_, CH_, 1, true, MW_, true>(st, N, staged, F, clampv, err, kA, kB, soft_part, Nf, kf, evA, evB, call.staged_lo)
#define DSAC_EX(NG_, CH_, MW_, F_) launch_reproject_st<NG_, CH_, 1, true, MW_, false, F_>(st, N, staged, F, clampv, err, kA, kB, soft_part, Nf, kf, evA, evB, nullptr, call.split)
#define DSAC_EXA(NG_, CH_, MW_) launch_reproject_any<NG_, CH_, MW_>(st, N, staged, F, clampv, err, kA, kB, soft_part, Nf, kf, evA, evB, call.split)
    switch (k.family) {
        case K2_FAM_NONE: return hipSuccess;  // an empty call
        case K2_FAM_VALU_SCALAR: return DSAC_VA(1, 32, false);
        case K2_FAM_VALU: case K2_FAM_HP: case K2_FAM_ST: case K2_FAM_PS:
            switch (k.id) {
#define K2_VA_(ID, PX, HT, SP) case ID: return DSAC_VA(PX, HT, SP);
#define K2_HP_(ID, HT, CH) case ID: return DSAC_HP(HT, CH);
#define K2_ST_(ID, NG, CH, WV, PW, MW) case ID: return DSAC_ST(NG, CH, WV, PW, MW);
#define K2_PS_(ID, NG) case ID: return DSAC_PS(NG);
                K2_FP32_IDS(K2_VA_, K2_HP_, K2_ST_, K2_PS_)
#undef K2_VA_
#undef K2_HP_
#undef K2_ST_
#undef K2_PS_
            }
            break;
        case K2_FAM_RECLO:
            switch (k.id) {
#define K2_LO_(ID, NG, CH, MW) case ID: return DSAC_LO(NG, CH, MW);
                K2_RECLO_IDS(K2_LO_)
#undef K2_LO_
            }
            break;
        case K2_FAM_EXACT_VEC:
#define K2_EX_(ID, NG, CH, MW, F_) if (k.ng == NG && k.ch == CH && k.minw == MW && k.exf == F_) return DSAC_EX(NG, CH, MW, F_);
            K2_EXACT_IDS(K2_EX_)
#undef K2_EX_
            // the 16-bit stores of the auto policy's two tiles: binary16 (EXF 3 / 4) and bfloat16 (5 / 6)
#define K2_AX_(NG, CH, MW)                                  \
            if (k.ng == NG && k.ch == CH && k.minw == MW)   \
                switch (k.exf) {                            \
                    case 3: return DSAC_EX(NG, CH, MW, 3);  \
                    case 4: return DSAC_EX(NG, CH, MW, 4);  \
                    case 5: return DSAC_EX(NG, CH, MW, 5);  \
                    case 6: return DSAC_EX(NG, CH, MW, 6);  \
                }
            K2_EXACT_AUTO_TILES(K2_AX_)
#undef K2_AX_
            break;
        case K2_FAM_EXACT_ANY:
#define K2_AX_(NG, CH, MW) if (k.ng == NG && k.ch == CH && k.minw == MW) return DSAC_EXA(NG, CH, MW);
            K2_EXACT_AUTO_TILES(K2_AX_)
#undef K2_AX_
            break;
        case K2_FAM_PRECISE: {
            const double kAd = (double)beta * 1.4426950408889634, kBd = -(double)beta * (double)tau * 1.4426950408889634;
            const int rec32 = (kf & K2_FLAG_REC32) ? 1 : 0;
            return k.ht == 32 ? launch_reproject_prec<32>(st, N, call.poses64, F, clampv, err, kAd, kBd, soft_part, Nf, evA, evB, rec32, call.diag)
                              : launch_reproject_prec<16>(st, N, call.poses64, F, clampv, err, kAd, kBd, soft_part, Nf, evA, evB, rec32, call.diag);
        }
    }
    return hipErrorInvalidValue;  // a kernel the plan never names
#undef DSAC_VA
#undef DSAC_HP
#undef DSAC_ST
#undef DSAC_PS
#undef DSAC_LO
#undef DSAC_EX
#undef DSAC_EXA
}

// --------------------------------------------------------------------------------------------------
// A workgroup of 16 waves per 64 hypotheses: lane = hypothesis (a wave reads 256 contiguous bytes of a partial row), wave w sums the rows
// t = w, w + 16, ... in fp64, then a fixed-order sum over the 16 waves -> deterministic.  (Rounds 1-2 ran one wave per hypothesis with the
// lanes striding over the rows: every lane touched its own 64-byte sector, fine for 300 rows, not for the 1200 of the one-wave tiles.)
constexpr int KR_WAVES = 16;
__global__ __launch_bounds__(KR_WAVES * 64) void k_reduce_soft(int N, int tiles, const float* __restrict__ part, double* __restrict__ soft) {
    __builtin_amdgcn_s_setprio(3);
    __shared__ double s_acc[KR_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.x * 64 + lane;
    double s = 0;
    if (h < N) {
#pragma unroll 16  // sixteen row reads in flight per wave (the adds stay in row order): 1 200 rows are 75 per wave, a chain of latencies at four
        for (int t = wave; t < tiles; t += KR_WAVES) s += (double)part[(size_t)t * N + h];
    }
    s_acc[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && h < N) {
        double tot = 0;
#pragma unroll
        for (int w = 0; w < KR_WAVES; w++) tot += s_acc[w][lane];
        soft[h] = tot;
    }
}

hipError_t reduce_soft(hipStream_t st, int N, int tiles, const float* soft_part, double* soft) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_reduce_soft, dim3((N + 63) / 64), dim3(KR_WAVES * 64), 0, st, N, tiles, soft_part, soft);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------
// K3: softmax (max-subtracted), Shannon entropy in bits, weighted pose average.  One workgroup, fp64,
// fixed reduction tree -> deterministic.  Replaces core/cnn_softam.h:535-553, :80-88, :1082-1094.
// --------------------------------------------------------------------------------------------------
constexpr int K3_THREADS = 256;

DM_INLINE double wave_allmax_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
DM_INLINE double wave_allsum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Two block-wide reductions in total: the maximum, then {sum e, sum e*log2 e, sum e*pose[0..5]} together.
// With S = sum e:  w_i = e_i / S,  entropy = log2 S - (sum e log2 e)/S,  avg = (sum e pose)/S.
__global__ __launch_bounds__(K3_THREADS) void k_softmax(int N, const double* __restrict__ scores, double scale, double* __restrict__ w,
                                                        double* __restrict__ entropy, const double* __restrict__ poses,
                                                        double* __restrict__ avg6) {
    __builtin_amdgcn_s_setprio(3);  // tiny latency-bound kernel, usually overlapped with a bandwidth-bound one
    {   // frame batch: workgroup f owns the N scores of frame f
        const size_t f = blockIdx.x;
        scores += f * N; w += f * N;
        if (entropy) entropy += f;
        if (poses) poses += f * N * 6;
        if (avg6) avg6 += f * 6;
    }
    __shared__ double s_m[K3_THREADS / 64];
    __shared__ double s_acc[K3_THREADS / 64][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool want_avg = poses && avg6;
    double m = -1.7976931348623157e308;
    for (int i = tid; i < N; i += K3_THREADS) m = fmax(m, scale * scores[i]);
    m = wave_allmax_d(m);
    if (lane == 0) s_m[wave] = m;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K3_THREADS / 64; k++) m = fmax(m, s_m[k]);
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < N; i += K3_THREADS) {
        const double x = scale * scores[i] - m;
        const double e = exp(x);
        w[i] = e;
        acc[0] += e;
        // e * log2(e); 0 when e is 0, like the reference's w > 0 test -- also for a score of -inf (a masked hypothesis), where e * x would be 0 * -inf = NaN.
        // The select sits on x, not on the product, so that the multiply-add below is the one finite scores have always had, bit for bit.
        const double xl = (e == 0.0) ? 0.0 : x;
        acc[1] += e * (xl * 1.4426950408889634);
        if (want_avg) {
#pragma unroll
            for (int k = 0; k < 6; k++) acc[2 + k] += e * poses[6 * (size_t)i + k];
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = wave_allsum_d(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) s_acc[wave][k] = acc[k];
    }
    __syncthreads();
    double tot[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        tot[k] = 0;
#pragma unroll
        for (int q = 0; q < K3_THREADS / 64; q++) tot[k] += s_acc[q][k];
    }
    const double S = tot[0];
    for (int i = tid; i < N; i += K3_THREADS) w[i] = w[i] / S;
    if (tid == 0) {
        if (entropy) *entropy = log2(S) - tot[1] / S;
        if (want_avg) {
#pragma unroll
            for (int k = 0; k < 6; k++) avg6[k] = tot[2 + k] / S;
        }
    }
}

hipError_t softmax(hipStream_t st, int N, const double* scores, double scale, double* w, double* entropy, const double* poses, double* avg6,
                   int frames) {
    if (N <= 0 || frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_softmax, dim3(frames), dim3(K3_THREADS), 0, st, N, scores, scale, w, entropy, poses, avg6);
    return hipGetLastError();
}

}  // namespace dk
