// k_rgbd.hip -- RGB-D localisation (include/dsac_hip.h, "RGB-D"): every cell carries a measured camera-frame point C_p next to its predicted scene
// coordinate X_p.  A hypothesis is the rigid alignment of three correspondences (dm::align3_lsq), an error is the 3D distance |R X + t - C| in mm, and
// the refinement is Horn's alignment over the whole map, re-weighted by the score's own sigmoid.  None of these kernels reads the camera intrinsics.
//
// The context's copy of the camera points is CANONICAL: a cell that is not VALID (C finite, C.z > 0, X finite) holds NaN in all three components, so
// every kernel below tells validity from one component (c == c) and needs no mask.
//
// This file is built with -ffp-contract=off (Makefile): the sampler's two paths (drawn and given sets) must round alike, and they do because they run
// the same instructions -- one kernel, one evaluation site.  Fused multiply-adds that are wanted are spelled out.
#include "kernels.h"
#include "dmath.h"
#include "soft_loop.h"

namespace dk {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

DM_INLINE f2 splat2(float a) { return f2{a, a}; }
DM_INLINE f2 pk_fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// sum over the wave, the same bits in every lane (each stage adds the same two partial sums in both partners)
DM_INLINE double wave_sum_d(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

DM_INLINE float row16_sum_f(float v) {  // sum over the 16 lanes of a DPP row, result in every lane
    int x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true));
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true));
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xf, 0xf, true));
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x140, 0xf, 0xf, true));
    return v;
}

constexpr int RGBD_NO_CELL = 0x7fffffff;

// ---- the measured points: canonical copy, VALID counts and the first VALID cell of every frame --------------------------------------------------
__global__ __launch_bounds__(64) void k_rgbd_meta_init(int frames, int32_t* __restrict__ meta) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f < frames) { meta[2 * f] = 0; meta[2 * f + 1] = RGBD_NO_CELL; }
}

// blockIdx.y = frame, 256 cells per workgroup.  meta[2 f] += VALID cells (integer adds: the count does not depend on their order), meta[2 f + 1] = the
// smallest VALID cell index
__global__ __launch_bounds__(256) void k_rgbd_canon(int P, const float* __restrict__ src, const float* __restrict__ xyz, long long xyz_stride, float* __restrict__ dst,
                                                    int32_t* __restrict__ meta) {
    const int f = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    if (p < P) {
        const float* s = src + ((size_t)f * P + p) * 3;
        const float* x = xyz + (long long)f * xyz_stride + (size_t)p * 3;
        const float cx = s[0], cy = s[1], cz = s[2];
        const float X = x[0], Y = x[1], Z = x[2];
        valid = (cx - cx == 0.f) && (cy - cy == 0.f) && (cz - cz == 0.f) && cz > 0.f && (X - X == 0.f) && (Y - Y == 0.f) && (Z - Z == 0.f);
        const float nan = __builtin_nanf("");
        float* d = dst + ((size_t)f * P + p) * 3;
        d[0] = valid ? cx : nan;
        d[1] = valid ? cy : nan;
        d[2] = valid ? cz : nan;
    }
    const unsigned long long m = __ballot(valid);
    if (m != 0ull && (threadIdx.x & 63) == 0) {
        atomicAdd(meta + 2 * f, (int)__popcll(m));
        atomicMin(meta + 2 * f + 1, (blockIdx.x * 256 + (int)(threadIdx.x & ~63u)) + (int)__builtin_ctzll(m));
    }
}

// ---- pose records of the scoring kernel: fp64 Rodrigues -> 12 floats R0 | t0, R1 | t1, R2 | t2 ---------------------------------------------------
__global__ __launch_bounds__(64) void k_rgbd_pose_prep(int N, const double* __restrict__ poses, float* __restrict__ rec) {
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= N) return;
    double r[3], R[9];
    dm::RodAux aux;
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = poses[(size_t)h * 6 + i];
    dm::rodrigues_R(r, R, aux);
    float* o = rec + (size_t)h * POSE_STRIDE;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        o[4 * i] = (float)R[3 * i];
        o[4 * i + 1] = (float)R[3 * i + 1];
        o[4 * i + 2] = (float)R[3 * i + 2];
        o[4 * i + 3] = (float)poses[(size_t)h * 6 + 3 + i];
    }
}

// ---- scoring: err[h][p] = min(|R_h X_p + t_h - C_p|, clamp), soft partials --------------------------------------------------------------------
// One-wave workgroups on a tile of 64 hypotheses x 256 cells, the shape K2's streaming form measured best (k_forward.hip, k_reproject_st).  Per group of
// 16 hypotheses and chunk of 64 cells: D = (R | t) . (X, Y, Z, 1) as v_mfma_f32_16x16x4_f32 (exact f32, bitwise an fmaf chain), accumulated onto -C, which
// a second matrix-core instruction places in the accumulator layout (A = -e_x / -e_y / -e_z in the lanes of k = 0 / 1 / 2, B = the camera point: exact,
// and no cross-lane traffic on the vector ALU).  Lane (g, c) then holds the difference vectors of hypotheses 4g .. 4g + 3 at the cells 4c .. 4c + 3 of
// the chunk: squared norms packed over hypothesis pairs, one v_sqrt_f32 per pair, min with the clamp (a NaN -- a cell that is not VALID -- gives the
// clamp), four 16-byte non-temporal stores with dword alignment (any map, any 4-byte-aligned err), dword stores for the 1-3 cells of a ragged end.
// The sigmoids of cells that are not VALID, and of the cells that pad the last chunk, are multiplied by 0: they add exactly 0.
// Tiles never straddle two frames: hypothesis tiles are counted per frame (tpf of them).
DM_INLINE f2 rgbd_soft2(f2 e, float kA, float kB) {
    const f2 t = pk_fma2(splat2(kA), e, splat2(kB));
    f2 ex;
    ex.x = __builtin_amdgcn_exp2f(t.x);
    ex.y = __builtin_amdgcn_exp2f(t.y);
    const f2 d = ex + splat2(1.0f);
    f2 s;
    s.x = __builtin_amdgcn_rcpf(d.x);
    s.y = __builtin_amdgcn_rcpf(d.y);
    return s;
}

constexpr int SC_NG = 4, SC_CHW = 4;  // 64 hypotheses x 256 cells per wave

template <bool ERR, bool SOFT>
__global__ __launch_bounds__(64, 2) void k_score_rgbd(const float* __restrict__ rec, const float* __restrict__ xyz, const float* __restrict__ cam, float* __restrict__ err,
                                                      float* __restrict__ soft_part, int N, int Nf, int tpf, int P, int PT, long long xyz_stride, float clampv,
                                                      float kA, float kB) {
    // XCD-aware order of K2's one-wave form: the workgroups b, b + 8, b + 16, b + 24 (same XCD, dispatched back to back) take adjacent cell tiles
    const int b = blockIdx.x;
    const int q = b >> 5, sub = (b >> 3) & 3, PTG = (PT + 31) >> 5;
    const int ht = q / PTG;
    const int pt = ((q % PTG) * 8 + (b & 7)) * 4 + sub;
    if (pt >= PT) return;
    const int frame = ht / tpf, hl0 = (ht - frame * tpf) * (16 * SC_NG);
    const int nh = min(16 * SC_NG, Nf - hl0);
    const int h0 = frame * Nf + hl0;
    xyz += (long long)frame * xyz_stride;
    cam += (size_t)frame * (size_t)P * 3;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;

    // B operands: coordinate g of cell 4c + m of every chunk (1 in the lanes of k = 3), and the camera point's component min(g, 2) -- the lanes of k = 3
    // meet a zero in A, and every lane can tell a VALID cell (c == c).  Cells beyond the map read the last cell and count as not VALID
    float Bx[SC_CHW][4], Bc[SC_CHW][4];
    int p0[SC_CHW];
    const int gc = min(g, 2);
#pragma unroll
    for (int ch = 0; ch < SC_CHW; ch++) {
        p0[ch] = (pt * SC_CHW + ch) * 64 + 4 * c;
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int p = p0[ch] + m, pc = min(p, P - 1);
            Bx[ch][m] = (g < 3) ? xyz[(size_t)pc * 3 + g] : 1.0f;
            const float cv = cam[(size_t)pc * 3 + gc];
            Bc[ch][m] = (p < P) ? cv : __builtin_nanf("");
        }
    }
    const float selx = (g == 0) ? -1.0f : 0.0f, sely = (g == 1) ? -1.0f : 0.0f, selz = (g == 2) ? -1.0f : 0.0f;
    const f4 z4 = {0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int gi = 0; gi < SC_NG; gi++) {
        if (16 * gi >= nh) break;
        const int hyp = min(16 * gi + c, nh - 1);  // beyond the ragged end: repeat the last hypothesis (never stored)
        const float* r = rec + (size_t)(h0 + hyp) * POSE_STRIDE + g;
        const float ax = r[0], ay = r[4], az = r[8];
        const int hyp0 = 16 * gi + 4 * g;
        f2 ssum[4] = {splat2(0.f), splat2(0.f), splat2(0.f), splat2(0.f)};
#pragma unroll
        for (int ch = 0; ch < SC_CHW; ch++) {
            if ((pt * SC_CHW + ch) * 64 >= P) break;  // wave-uniform: the chunk lies beyond the map
            f2 qq[4][2];
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const f4 cx4 = __builtin_amdgcn_mfma_f32_16x16x4f32(selx, Bc[ch][m], z4, 0, 0, 0);
                const f4 cy4 = __builtin_amdgcn_mfma_f32_16x16x4f32(sely, Bc[ch][m], z4, 0, 0, 0);
                const f4 cz4 = __builtin_amdgcn_mfma_f32_16x16x4f32(selz, Bc[ch][m], z4, 0, 0, 0);
                const f4 dx = __builtin_amdgcn_mfma_f32_16x16x4f32(ax, Bx[ch][m], cx4, 0, 0, 0);
                const f4 dy = __builtin_amdgcn_mfma_f32_16x16x4f32(ay, Bx[ch][m], cy4, 0, 0, 0);
                const f4 dz = __builtin_amdgcn_mfma_f32_16x16x4f32(az, Bx[ch][m], cz4, 0, 0, 0);
#pragma unroll
                for (int pr = 0; pr < 2; pr++) {
                    const f2 x = pr ? f2{dx.z, dx.w} : f2{dx.x, dx.y};
                    const f2 y = pr ? f2{dy.z, dy.w} : f2{dy.x, dy.y};
                    const f2 z = pr ? f2{dz.z, dz.w} : f2{dz.x, dz.y};
                    qq[m][pr] = pk_fma2(z, z, pk_fma2(y, y, x * x));
                }
            }
            f4 ev[4];
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int pr = rr >> 1;
                ev[rr].x = fminf(__builtin_amdgcn_sqrtf((rr & 1) ? qq[0][pr].y : qq[0][pr].x), clampv);
                ev[rr].y = fminf(__builtin_amdgcn_sqrtf((rr & 1) ? qq[1][pr].y : qq[1][pr].x), clampv);
                ev[rr].z = fminf(__builtin_amdgcn_sqrtf((rr & 1) ? qq[2][pr].y : qq[2][pr].x), clampv);
                ev[rr].w = fminf(__builtin_amdgcn_sqrtf((rr & 1) ? qq[3][pr].y : qq[3][pr].x), clampv);
            }
            if (SOFT) {
                const f2 m01 = {Bc[ch][0] == Bc[ch][0] ? 1.0f : 0.0f, Bc[ch][1] == Bc[ch][1] ? 1.0f : 0.0f};
                const f2 m23 = {Bc[ch][2] == Bc[ch][2] ? 1.0f : 0.0f, Bc[ch][3] == Bc[ch][3] ? 1.0f : 0.0f};
#pragma unroll
                for (int rr = 0; rr < 4; rr++)
                    ssum[rr] += pk_fma2(rgbd_soft2(f2{ev[rr].x, ev[rr].y}, kA, kB), m01, rgbd_soft2(f2{ev[rr].z, ev[rr].w}, kA, kB) * m23);
            }
            if (ERR && p0[ch] < P) {
                // buffer stores: a wave-uniform row base in a scalar resource + a scalar row offset + a 32-bit lane offset (the launcher bounds 64 rows of the
                // map to 2^32 bytes)
                const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(err + (size_t)(h0 + 16 * gi) * P, 0, 0xffffffffu, 0x00020000);
                const unsigned loff = ((unsigned)(4 * g) * (unsigned)P + (unsigned)p0[ch]) * 4u;
                const int nv = P - p0[ch];
                if (nv >= 4) {
                    if (nh == 16 * SC_NG) {
#pragma unroll
                        for (int rr = 0; rr < 4; rr++) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, ev[rr]), rsrc, loff, (unsigned)rr * (unsigned)P * 4u, 2);
                    } else {
#pragma unroll
                        for (int rr = 0; rr < 4; rr++)
                            if (hyp0 + rr < nh) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, ev[rr]), rsrc, loff, (unsigned)rr * (unsigned)P * 4u, 2);
                    }
                } else {
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) {
                        if (hyp0 + rr >= nh) continue;
                        const unsigned soff = (unsigned)rr * (unsigned)P * 4u;
                        const float ex = ev[rr].x, ey = ev[rr].y, ez = ev[rr].z;
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ex), rsrc, loff, soff, 2);
                        if (nv > 1) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ey), rsrc, loff + 4u, soff, 2);
                        if (nv > 2) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ez), rsrc, loff + 8u, soff, 2);
                    }
                }
            }
        }
        if (SOFT) {
            const float s0 = row16_sum_f(ssum[0].x + ssum[0].y), s1 = row16_sum_f(ssum[1].x + ssum[1].y);
            const float s2 = row16_sum_f(ssum[2].x + ssum[2].y), s3 = row16_sum_f(ssum[3].x + ssum[3].y);
            if (c == 0) {
                float* dst = soft_part + (size_t)pt * N + h0 + hyp0;
                if (hyp0 + 0 < nh) dst[0] = s0;
                if (hyp0 + 1 < nh) dst[1] = s1;
                if (hyp0 + 2 < nh) dst[2] = s2;
                if (hyp0 + 3 < nh) dst[3] = s3;
            }
        }
    }
}

// ---- sampling: three cells, Horn's three-point alignment in closed form, the 3D check ----------------------------------------------------------
// Candidate walk of attempt a (dsac_hip.h, "Sampling RNG"): k = 0 .. 31, a candidate that is not VALID or already in the set is skipped.
DM_INLINE bool rgbd_draw3(uint64_t key, uint32_t attempt, uint32_t W, uint32_t H, const float* __restrict__ cam, int& c0, int& c1, int& c2) {
    int n = 0, s0 = 0, s1 = 0, s2 = 0;  // selects, not an indexed triple: the set stays in registers
    for (uint32_t k = 0; k < 32 && n < 3; k++) {
        const int cell = dm::draw_cell(key, attempt, k, W, H);
        const float v = cam[(size_t)cell * 3];
        const bool dup = (n > 0 && cell == s0) || (n > 1 && cell == s1);
        const bool take = v == v && !dup;
        s0 = (take && n == 0) ? cell : s0;
        s1 = (take && n == 1) ? cell : s1;
        s2 = (take && n == 2) ? cell : s2;
        n += take ? 1 : 0;
    }
    c0 = s0; c1 = s1; c2 = s2;
    return n == 3;
}

// The draw is a policy of the kernel (template parameter DRAW), as it is of k_sample: where the three cells of an attempt come from is all that differs
// between the uniform build and the guided one (dsac_set_sampling_weights_rgbd); the evaluation, the ballot and the failure rows are one text.
//   bind(P, frame): once per wave, drawn sets only;  empty(cam_meta, frame): no attempt of this frame can draw three cells;  draw(): the set of an attempt.
struct DrawUniform3 {
    DM_INLINE void bind(int, int) {}
    DM_INLINE bool empty(const int32_t* __restrict__ cam_meta, int frame) const { return cam_meta[2 * frame] < 3; }
    DM_INLINE bool draw(uint64_t key, uint32_t attempt, uint32_t W, uint32_t H, const float* __restrict__ cam, int& c0, int& c1, int& c2) const {
        return rgbd_draw3(key, attempt, W, H, cam, c0, c1, c2);
    }
};

// Guided draw: candidate k is the cell of t = floor(v * T' / 2^64) in the frame's table of the MASKED weights (DrawGuided in k_sample.hip has the rule and
// the measurements; dm::table_cells the search).  The table holds no mass on a cell that is not VALID, so no candidate needs a VALID load.  The first three
// candidates are searched side by side -- their dependent loads overlap --; only when two of them coincide does the walk go on candidate by candidate, from
// k = 0 with the three cells already found, so the set is the sequential walk's.  One wave per workgroup: it holds ONE frame's coarse level in LDS.
struct DrawGuided3 {
    const uint64_t* cdf;     // frames x P
    const GuideMeta* meta;   // frames
    const uint64_t* coarse;  // frames x K, K = ceil(P / 2^shift)
    int shift;
    const uint64_t* C;
    const uint64_t* L;       // the frame's coarse level in LDS
    uint64_t T;
    int P, n, K;
    DM_INLINE void bind(int P_, int frame) {
        __shared__ uint64_t s_coarse[GUIDE_COARSE_MAX];
        frame = __builtin_amdgcn_readfirstlane(frame);  // one hypothesis per wave: the table's rows are scalar loads
        P = P_;
        K = (P + (1 << shift) - 1) >> shift;
        C = cdf + (size_t)frame * (size_t)P;
        T = meta[frame].T;
        n = meta[frame].n;
        L = s_coarse;
        if (n >= 3) {  // uniform over the workgroup
            const uint64_t* cf = coarse + (size_t)frame * (size_t)K;
            for (int i = threadIdx.x; i < K; i += blockDim.x) s_coarse[i] = cf[i];
            __syncthreads();
        }
    }
    DM_INLINE bool empty(const int32_t*, int) const { return n < 3; }
    DM_INLINE uint64_t target(uint64_t key, uint32_t attempt, uint32_t k) const { return __umul64hi(dm::mix64(key + (((uint64_t)attempt << 16) | k)), T); }
    DM_INLINE bool draw(uint64_t key, uint32_t attempt, uint32_t, uint32_t, const float*, int& c0, int& c1, int& c2) const {
        uint64_t t[3];
        int32_t c[3];
#pragma unroll
        for (int j = 0; j < 3; j++) t[j] = target(key, attempt, (uint32_t)j);
        dm::table_cells<3>(L, K, C, P, shift, t, c);
        c0 = c[0]; c1 = c[1]; c2 = c[2];
        if (c0 != c1 && c0 != c2 && c1 != c2) return true;
        int m = 0, s0 = 0, s1 = 0, s2 = 0;
        for (uint32_t k = 0; k < 32 && m < 3; k++) {
            int32_t cell = k == 0 ? c[0] : k == 1 ? c[1] : c[2];
            if (k >= 3) {
                const uint64_t tk = target(key, attempt, k);
                dm::table_cells<1>(L, K, C, P, shift, &tk, &cell);
            }
            const bool take = !((m > 0 && cell == s0) || (m > 1 && cell == s1));
            s0 = (take && m == 0) ? cell : s0;
            s1 = (take && m == 1) ? cell : s1;
            s2 = (take && m == 2) ? cell : s2;
            m += take ? 1 : 0;
        }
        c0 = s0; c1 = s1; c2 = s2;
        return m == 3;
    }
};

// One kernel for both paths, ONE evaluation site: a lane evaluates one candidate set per round.
//   drawn sets (sets_in == nullptr): workgroup = one wave = hypothesis blockIdx.x; lane l of round r evaluates attempt 64 r + l; the lowest accepted lane of
//   the first round that has one wins (ballot).
//   given sets: lane l of workgroup w evaluates the set of hypothesis 64 w + l, once.
// DRAW / TAB: the draw policy and what it is built from -- nothing for the uniform build, whose argument list is the one it always had, and the table (cdf,
// per-frame records, coarse level, its shift) for the guided one, which is launched on drawn sets only.
template <class DRAW = DrawUniform3, class... TAB>
__global__ __launch_bounds__(64) void k_sample_rgbd(int N, int Nf, uint64_t seed, int seed_stride, const int32_t* __restrict__ sets_in, const float* __restrict__ xyz,
                                                    long long xyz_stride, const float* __restrict__ cam, const int32_t* __restrict__ meta, int P, int W, int H,
                                                    double thr, int max_tries, double* __restrict__ poses, int32_t* __restrict__ sets_out, uint8_t* __restrict__ ok,
                                                    TAB... tab) {
    DRAW D{tab...};
    const int lane = threadIdx.x & 63;
    const bool given = sets_in != nullptr;
    const int h = given ? blockIdx.x * 64 + lane : blockIdx.x;
    const bool mine = h < N;
    uint64_t key = 0;
    if (!given) {
        const int frame = Nf > 0 ? h / Nf : 0;
        const int hl = Nf > 0 ? h - frame * Nf : h;
        xyz += (long long)frame * xyz_stride;
        cam += (size_t)frame * (size_t)P * 3;
        key = dm::hyp_key(seed + (uint64_t)frame * (uint64_t)seed_stride, (uint32_t)hl);
        D.bind(P, frame);
        if (D.empty(meta, frame)) {  // no attempt of this frame can draw three cells
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 6; i++) poses[(size_t)h * 6 + i] = 0.0;
                sets_out[(size_t)h * 3] = sets_out[(size_t)h * 3 + 1] = sets_out[(size_t)h * 3 + 2] = 0;
                ok[h] = 0;
            }
            return;
        }
    }
    const int rounds = given ? 1 : (max_tries + 63) / 64;
    for (int round = 0; round < rounds; round++) {
        int c0 = 0, c1 = 0, c2 = 0;
        bool have;
        if (given) {
            if (mine) { c0 = sets_in[(size_t)h * 3]; c1 = sets_in[(size_t)h * 3 + 1]; c2 = sets_in[(size_t)h * 3 + 2]; }
            have = mine && c0 >= 0 && c0 < P && c1 >= 0 && c1 < P && c2 >= 0 && c2 < P && c0 != c1 && c0 != c2 && c1 != c2;
            if (have) {
                const float v0 = cam[(size_t)c0 * 3], v1 = cam[(size_t)c1 * 3], v2 = cam[(size_t)c2 * 3];
                have = v0 == v0 && v1 == v1 && v2 == v2;
            }
        } else {
            const int a = round * 64 + lane;
            have = a < max_tries && D.draw(key, (uint32_t)a, (uint32_t)W, (uint32_t)H, cam, c0, c1, c2);
        }
        // the evaluation (lanes without a set evaluate cell 0 three times and are not accepted)
        const int e0 = have ? c0 : 0, e1 = have ? c1 : 0, e2 = have ? c2 : 0;
        double X[3][3], M[3][3], R[9], T[3], pose[6];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            X[0][j] = (double)xyz[(size_t)e0 * 3 + j]; M[0][j] = (double)cam[(size_t)e0 * 3 + j];
            X[1][j] = (double)xyz[(size_t)e1 * 3 + j]; M[1][j] = (double)cam[(size_t)e1 * 3 + j];
            X[2][j] = (double)xyz[(size_t)e2 * 3 + j]; M[2][j] = (double)cam[(size_t)e2 * 3 + j];
        }
        dm::align3_lsq(M, X, R, T);
        dm::rodrigues_m2v(R, pose);
        pose[3] = T[0]; pose[4] = T[1]; pose[5] = T[2];
        bool acc = have;
#pragma unroll
        for (int i = 0; i < 6; i++) acc = acc && finite_d(pose[i]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double dx = R[0] * X[k][0] + R[1] * X[k][1] + R[2] * X[k][2] + T[0] - M[k][0];
            const double dy = R[3] * X[k][0] + R[4] * X[k][1] + R[5] * X[k][2] + T[1] - M[k][1];
            const double dz = R[6] * X[k][0] + R[7] * X[k][1] + R[8] * X[k][2] + T[2] - M[k][2];
            acc = acc && (sqrt(dx * dx + dy * dy + dz * dz) < thr);
        }
        bool writer;
        if (given) writer = mine;
        else {
            const unsigned long long m = __ballot(acc);
            writer = m != 0ull && lane == (int)__builtin_ctzll(m);
            if (m == 0ull) continue;
        }
        if (writer) {
#pragma unroll
            for (int i = 0; i < 6; i++) poses[(size_t)h * 6 + i] = acc ? pose[i] : 0.0;
            sets_out[(size_t)h * 3] = c0; sets_out[(size_t)h * 3 + 1] = c1; sets_out[(size_t)h * 3 + 2] = c2;
            ok[h] = acc ? 1 : 0;
        }
        return;
    }
    // drawn sets, no attempt accepted: the set of the last attempt if it drew three cells, else zeros
    if (lane == 0) {
        int c0, c1, c2;
        if (!D.draw(key, (uint32_t)(max_tries - 1), (uint32_t)W, (uint32_t)H, cam, c0, c1, c2)) c0 = c1 = c2 = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) poses[(size_t)h * 6 + i] = 0.0;
        sets_out[(size_t)h * 3] = c0; sets_out[(size_t)h * 3 + 1] = c1; sets_out[(size_t)h * 3 + 2] = c2;
        ok[h] = 0;
    }
}

// the masked weights of guided RGB-D sampling (dsac_set_sampling_weights_rgbd): w' = w where the cell is VALID, 0 elsewhere; the table build of
// dsac_set_sampling_weights (k_sample.hip, guide_build) then runs on w'.  A lane per cell over all frames
__global__ __launch_bounds__(256) void k_rgbd_mask_weights(long long cells, const float* __restrict__ w, const float* __restrict__ cam, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const float c = cam[(size_t)i * 3];
    out[i] = (c == c) ? w[i] : 0.0f;  // the canonical copy: a cell that is not VALID holds NaN
}

// ---- refinement: Horn's alignment over the whole map, re-weighted by the score's sigmoid ---------------------------------------------------------
// The loop of dsac_refine_soft (soft_loop.h) with another pass and another step: split form, a pass kernel on cell chunks x problems whose 16 sums go to
// scratch and the one-wave step kernel that adds them in chunk order, decides and moves the pose; max_iters + 1 of each, no host round trip, no
// floating-point atomics.  The sums are taken about the frame's first VALID cell (X0, C0): x = X - X0, c = C - C0.
constexpr int RG_NACC = 16;  // S, sum w x (3), sum w c (3), sum w x c^T (9, row = x)

// (X0, C0) of a frame whose first VALID cell is `first` (xyz, cam: the frame's); zeros where the frame has none
DM_INLINE void rg_origin(const float* __restrict__ xyz, const float* __restrict__ cam, int first, int P, double X0[3], double C0[3]) {
#pragma unroll
    for (int j = 0; j < 3; j++) X0[j] = C0[j] = 0.0;
    if (first < P) {
#pragma unroll
        for (int j = 0; j < 3; j++) { X0[j] = (double)xyz[(size_t)first * 3 + j]; C0[j] = (double)cam[(size_t)first * 3 + j]; }
    }
}

__global__ __launch_bounds__(64) void k_rgbd_pass(int B, const double* __restrict__ poses, int pose_stride, const int32_t* __restrict__ done,
                                                  const int32_t* __restrict__ frame_of, int per_frame, int frames, int chunk, int nchunks, double tau, double beta,
                                                  double cut, const float* __restrict__ xyz, long long xyz_stride, const float* __restrict__ cam,
                                                  const int32_t* __restrict__ meta, int P, double* __restrict__ part) {
    const int b = blockIdx.x / nchunks, ck = blockIdx.x - b * nchunks;
    if (b >= B) return;
    if (done && done[b]) return;  // a finished problem: one flag load
    const int lane = threadIdx.x & 63;
    const int f = soft_problem_frame(frames, frame_of, per_frame, b);
    xyz += (long long)f * xyz_stride;
    cam += (size_t)f * (size_t)P * 3;
    double pose[6], R[9];
#pragma unroll
    for (int i = 0; i < 6; i++) pose[i] = poses[(size_t)b * pose_stride + i];
    dm::RodAux aux;
    dm::rodrigues_R(pose, R, aux);
    double X0[3], C0[3];
    rg_origin(xyz, cam, meta[2 * f + 1], P, X0, C0);
    double acc[RG_NACC];
#pragma unroll
    for (int i = 0; i < RG_NACC; i++) acc[i] = 0.0;
    const int begin = ck * chunk, end = min(P, begin + chunk);
    for (int base = begin; base < end; base += 64) {
        const int p = base + lane;
        const int pc = p < end ? p : end - 1;
        const double Xx = (double)xyz[(size_t)pc * 3], Xy = (double)xyz[(size_t)pc * 3 + 1], Xz = (double)xyz[(size_t)pc * 3 + 2];
        const double Cx = (double)cam[(size_t)pc * 3], Cy = (double)cam[(size_t)pc * 3 + 1], Cz = (double)cam[(size_t)pc * 3 + 2];
        const double dx = R[0] * Xx + R[1] * Xy + R[2] * Xz + pose[3] - Cx;
        const double dy = R[3] * Xx + R[4] * Xy + R[5] * Xz + pose[4] - Cy;
        const double dz = R[6] * Xx + R[7] * Xy + R[8] * Xz + pose[5] - Cz;
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        const bool live = p < end && d < cut;  // false for a NaN (a cell that is not VALID, a non-finite pose); an infinite d is not below a finite cut
        if (__ballot(live) == 0ull) continue;
        const double w = live ? 1.0 / (1.0 + exp(-beta * (tau - d))) : 0.0;
        const double x[3] = {live ? Xx - X0[0] : 0.0, live ? Xy - X0[1] : 0.0, live ? Xz - X0[2] : 0.0};
        const double c[3] = {live ? Cx - C0[0] : 0.0, live ? Cy - C0[1] : 0.0, live ? Cz - C0[2] : 0.0};
        acc[0] += w;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double wx = w * x[a];
            acc[1 + a] += wx;
            acc[4 + a] = fma(w, c[a], acc[4 + a]);
#pragma unroll
            for (int j = 0; j < 3; j++) acc[7 + 3 * a + j] = fma(wx, c[j], acc[7 + 3 * a + j]);
        }
    }
    double* dst = part + ((size_t)b * nchunks + ck) * RG_NACC;
#pragma unroll
    for (int i = 0; i < RG_NACC; i++) {
        const double s = wave_sum_d(acc[i]);
        if (lane == 0) dst[i] = s;
    }
}

// The RGB-D path's policy of the loop: 16 sums, Horn's closed form about (X0, C0) -- which the step loads as the pass does --, the length of a move the
// norm of h' - h.  Host side: what the pass launch takes
struct SoftRgbd {
    static constexpr int NACC = RG_NACC, S_AT = 0;
    struct Src {
        const int32_t* frame_of;
        int per_frame, frames;
        const float* xyz;
        long long xyz_stride;
        const float* cam;
        const int32_t* meta;
        int P;
    };
    struct RgOrigin { double X0[3], C0[3]; };
    static DM_INLINE RgOrigin load(const Src& s, int b) {
        const int f = soft_problem_frame(s.frames, s.frame_of, s.per_frame, b);
        RgOrigin o;
        rg_origin(s.xyz + (long long)f * s.xyz_stride, s.cam + (size_t)f * (size_t)s.P * 3, s.meta[2 * f + 1], s.P, o.X0, o.C0);
        return o;
    }
    static DM_INLINE bool step(const double* tot, const double h[6], const RgOrigin& o, double hn[6], double& len2);
    double tau, beta, cut;
    Src src;
    void pass(hipStream_t st, unsigned grid, const SoftGeom& geom, int B, const double* poses, int pose_stride, const int32_t* done, double* part) const {
        hipLaunchKernelGGL(k_rgbd_pass, dim3(grid), dim3(64), 0, st, B, poses, pose_stride, done, src.frame_of, src.per_frame, src.frames, geom.chunk, geom.nchunks, tau,
                           beta, cut, src.xyz, src.xyz_stride, src.cam, src.meta, src.P, part);
    }
};

DM_INLINE bool SoftRgbd::step(const double* tot, const double h[6], const RgOrigin& o, double hn[6], double& len2) {
    const double Sn = tot[0];
    // the step: weighted means, cross-covariance K (row = scene axis, column = camera axis), Horn's 4 x 4 matrix as dm::align3_horn builds it
    const double inv = 1.0 / Sn;
    double xm[3], cm[3], s[9];
#pragma unroll
    for (int a = 0; a < 3; a++) { xm[a] = tot[1 + a] * inv; cm[a] = tot[4 + a] * inv; }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int j = 0; j < 3; j++) s[a * 3 + j] = tot[7 + 3 * a + j] * inv - xm[a] * cm[j];
    double Q[16], ev[4], U[16];
    Q[0] = s[0] + s[4] + s[8];
    Q[5] = s[0] - s[4] - s[8];
    Q[10] = s[4] - s[8] - s[0];
    Q[15] = s[8] - s[0] - s[4];
    Q[4] = Q[1] = s[5] - s[7];
    Q[8] = Q[2] = s[6] - s[2];
    Q[12] = Q[3] = s[1] - s[3];
    Q[9] = Q[6] = s[3] + s[1];
    Q[13] = Q[7] = s[6] + s[2];
    Q[14] = Q[11] = s[7] + s[5];
    dm::jacobi4(Q, ev, U);
    // eigenvector of the largest eigenvalue (first maximum wins), and the second largest eigenvalue
    double l1 = ev[0], q0 = U[0], q1 = U[4], q2 = U[8], q3 = U[12];
    int i1 = 0;
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (ev[i] > l1) { l1 = ev[i]; i1 = i; q0 = U[i]; q1 = U[4 + i]; q2 = U[8 + i]; q3 = U[12 + i]; }
    double l2 = -1.7976931348623157e308;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (i != i1 && ev[i] > l2) l2 = ev[i];
    const double qn = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    q0 *= qn; q1 *= qn; q2 *= qn; q3 *= qn;
    const double q02 = q0 * q0, q12 = q1 * q1, q22 = q2 * q2, q32 = q3 * q3;
    const double q0_1 = q0 * q1, q0_2 = q0 * q2, q0_3 = q0 * q3, q1_2 = q1 * q2, q1_3 = q1 * q3, q2_3 = q2 * q3;
    double Rn[9];
    Rn[0] = q02 + q12 - q22 - q32; Rn[1] = 2. * (q1_2 - q0_3); Rn[2] = 2. * (q1_3 + q0_2);
    Rn[3] = 2. * (q1_2 + q0_3); Rn[4] = q02 + q22 - q12 - q32; Rn[5] = 2. * (q2_3 - q0_1);
    Rn[6] = 2. * (q1_3 - q0_2); Rn[7] = 2. * (q2_3 + q0_1); Rn[8] = q02 + q32 - q12 - q22;
    dm::rodrigues_m2v(Rn, hn);
    const double Xb[3] = {o.X0[0] + xm[0], o.X0[1] + xm[1], o.X0[2] + xm[2]};
#pragma unroll
    for (int i = 0; i < 3; i++) hn[3 + i] = (o.C0[i] + cm[i]) - (Rn[i * 3] * Xb[0] + Rn[i * 3 + 1] * Xb[1] + Rn[i * 3 + 2] * Xb[2]);
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; i++) fin = fin && finite_d(Rn[i]);
#pragma unroll
    for (int i = 0; i < 6; i++) fin = fin && finite_d(hn[i]);
    if (!fin || !(l1 - l2 > 1e-9 * l1)) return false;
    len2 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) { const double d = hn[i] - h[i]; len2 += d * d; }
    return true;
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------
hipError_t rgbd_set_points(hipStream_t st, const float* src, const FrameDev& F, float* cam_copy, int32_t* meta) {
    const int frames = F.frames > 1 ? F.frames : 1;
    if (F.P < 1 || frames > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rgbd_meta_init, dim3((unsigned)((frames + 63) / 64)), dim3(64), 0, st, frames, meta);
    hipLaunchKernelGGL(k_rgbd_canon, dim3((unsigned)((F.P + 255) / 256), (unsigned)frames), dim3(256), 0, st, F.P, src, F.xyz, F.xyz_stride, cam_copy, meta);
    return hipGetLastError();
}

hipError_t rgbd_sample(hipStream_t st, int N, uint64_t seed, const int32_t* sets_in, const FrameDev& F, const float* cam, const int32_t* meta, double thr,
                       int max_tries, double* poses, int32_t* sets_out, uint8_t* ok, int Nf, const GuideView* guide) {
    if (N <= 0) return hipSuccess;
    const unsigned grid = sets_in ? (unsigned)((N + 63) / 64) : (unsigned)N;
    if (guide && !sets_in) {  // given sets are evaluated by the uniform build: the weights do not touch them
        if (!guide->cdf || !guide->meta || !guide->coarse) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_sample_rgbd<DrawGuided3, const uint64_t*, const GuideMeta*, const uint64_t*, int>), dim3(grid), dim3(64), 0, st, N, Nf, seed, F.seed_stride,
                           sets_in, F.xyz, F.xyz_stride, cam, meta, F.P, F.W, F.H, thr, max_tries, poses, sets_out, ok, guide->cdf, guide->meta, guide->coarse,
                           guide_coarse_shift(F.P));
    } else {
        hipLaunchKernelGGL((k_sample_rgbd<>), dim3(grid), dim3(64), 0, st, N, Nf, seed, F.seed_stride, sets_in, F.xyz, F.xyz_stride, cam, meta, F.P, F.W, F.H, thr,
                           max_tries, poses, sets_out, ok);
    }
    return hipGetLastError();
}

hipError_t rgbd_mask_weights(hipStream_t st, int frames, int P, const float* w, const float* cam, float* out) {
    const long long cells = (long long)frames * P;
    if (cells <= 0) return hipSuccess;
    if ((cells + 255) / 256 > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rgbd_mask_weights, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, cells, w, cam, out);
    return hipGetLastError();
}

int rgbd_score_tiles(int P) { return (P + 64 * SC_CHW - 1) / (64 * SC_CHW); }

hipError_t rgbd_score(hipStream_t st, int N, const double* poses, float* rec, const FrameDev& F, const float* cam, float clampv, float* err, float tau, float beta,
                      float* soft_part, double* soft, int Nf) {
    if (N <= 0) return hipSuccess;
    if ((long long)F.P * 4 * 16 * SC_NG >= (1ll << 32)) return hipErrorInvalidValue;  // the 32-bit lane offsets of a tile's 64 rows
    const int nf = Nf > 0 ? Nf : N, frames = N / nf;
    const int tpf = (nf + 16 * SC_NG - 1) / (16 * SC_NG);
    const int PT = rgbd_score_tiles(F.P), PTG = (PT + 31) >> 5;
    const long long grid = (long long)frames * tpf * PTG * 32;
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rgbd_pose_prep, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, N, poses, rec);
    const float LOG2E = 1.4426950408889634f;
    const float kA = beta * LOG2E, kB = -beta * tau * LOG2E;
    const bool want_soft = soft != nullptr;
#define RGBD_SCORE(E, S)                                                                                                                                   \
    hipLaunchKernelGGL((k_score_rgbd<E, S>), dim3((unsigned)grid), dim3(64), 0, st, rec, F.xyz, cam, err, soft_part, N, nf, tpf, F.P, PT, F.xyz_stride, clampv, \
                       kA, kB)
    if (err && want_soft) RGBD_SCORE(true, true);
    else if (err) RGBD_SCORE(true, false);
    else if (want_soft) RGBD_SCORE(false, true);
#undef RGBD_SCORE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !want_soft) return e;
    return reduce_soft(st, N, PT, soft_part, soft);
}

size_t rgbd_refine_scratch_bytes(int B, const SoftGeom& g) { return soft_loop_bytes(RG_NACC, B, g); }

hipError_t rgbd_refine(hipStream_t st, int B, const double* init_poses, const int32_t* frame_of, int per_frame, double tau, double beta, double cut, double min_soft,
                       int max_iters, double step_tol, const SoftGeom& geom, void* scratch, double* out_poses, double* soft_out, int32_t* iters_out,
                       int32_t* status_out, const FrameDev& F, const float* cam, const int32_t* meta) {
    if (B < 1 || F.P < 1 || max_iters < 1 || (long long)B * geom.nchunks > 0x7fffffffll) return hipErrorInvalidValue;
    const SoftRgbd pol{tau, beta, cut, {frame_of, per_frame, F.frames > 1 ? F.frames : 1, F.xyz, F.xyz_stride, cam, meta, F.P}};
    return soft_loop(st, pol, B, init_poses, min_soft, max_iters, step_tol, geom, scratch, out_poses, soft_out, iters_out, status_out);
}

}  // namespace dk
