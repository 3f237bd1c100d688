// K2 lab (round 3): times the forms of dk::reproject on the bench shape (16 frames x 256 hypotheses x 640x480, error images + soft-inlier
// sums) without Python, and checks every form against a reference form (max |err - err_ref| over the whole volume, max rel diff of the
// reduced soft sums).  Usage: k2_lab [frames=16] [variant list ...]   (variant v, or v:flags)
#include "../../dsac_amd/csrc/k_forward.hip"
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include <string>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

__global__ void k_maxdiff(const float* a, const float* b, size_t n, float* out) {
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(a[i] - b[i]));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned*>(out), __float_as_uint(m));  // m >= 0: the bit pattern orders like the value
}

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s; }
static float urand(unsigned& s) { return (lcg(s) >> 8) * (1.0f / 16777216.0f); }

int main(int argc, char** argv) {
    const int frames = argc > 1 ? atoi(argv[1]) : 16;
    const int Nf = 256, H = 480, W = 640, P = H * W, N = frames * Nf;
    std::vector<std::string> vars;
    for (int i = 2; i < argc; i++) vars.push_back(argv[i]);
    if (vars.empty()) vars = {"21", "24", "40", "41", "42", "43", "44", "45", "46", "47", "48", "49"};
    unsigned seed = 12345u;
    // scene: points in front of the camera, most of them re-projecting near their pixel under a near-identity pose
    std::vector<float> xyz((size_t)frames * P * 3), staged((size_t)N * 12);
    for (int f = 0; f < frames; f++)
        for (int p = 0; p < P; p++) {
            const int y = p / W, x = p % W;
            const float z = 1500.f + 2000.f * urand(seed);
            float* o = &xyz[((size_t)f * P + p) * 3];
            o[0] = (x - 320.f) / 525.f * z + 30.f * (urand(seed) - 0.5f);
            o[1] = (y - 240.f) / 525.f * z + 30.f * (urand(seed) - 0.5f);
            o[2] = z;
        }
    for (int h = 0; h < N; h++) {
        const float a = 0.05f * (urand(seed) - 0.5f), b = 0.05f * (urand(seed) - 0.5f), c = 0.05f * (urand(seed) - 0.5f);
        // small-angle rotation, not exactly orthonormal: irrelevant for the arithmetic under test
        const float R[9] = {1, -c, b, c, 1, -a, -b, a, 1};
        const float t[3] = {40.f * (urand(seed) - 0.5f), 40.f * (urand(seed) - 0.5f), 60.f * (urand(seed) - 0.5f)};
        float* o = &staged[(size_t)h * 12];
        for (int k = 0; k < 3; k++) { o[k] = 525.f * R[k]; o[4 + k] = 525.f * R[3 + k]; o[8 + k] = R[6 + k]; }
        o[3] = 525.f * t[0]; o[7] = 525.f * t[1]; o[11] = t[2];
    }
    if (getenv("K2LAB_CHESS")) {  // the bench's scene: one chess-like frame (dsac_amd/synth.py) for all frames, 256 sampled hypotheses repeated
        FILE* f = fopen("scripts/micro/frame_chess.bin", "rb");
        std::vector<float> one((size_t)P * 3);
        if (!f || fread(one.data(), 4, one.size(), f) != one.size()) { printf("cannot read scripts/micro/frame_chess.bin\n"); return 1; }
        fclose(f);
        for (int fr = 0; fr < frames; fr++) std::copy(one.begin(), one.end(), xyz.begin() + (size_t)fr * P * 3);
        f = fopen("scripts/micro/poses_chess.bin", "rb");
        std::vector<float> ps(256 * 12);
        if (!f || fread(ps.data(), 4, ps.size(), f) != ps.size()) { printf("cannot read scripts/micro/poses_chess.bin\n"); return 1; }
        fclose(f);
        for (int h = 0; h < N; h++) std::copy(ps.begin() + (h % 256) * 12, ps.begin() + (h % 256) * 12 + 12, staged.begin() + (size_t)h * 12);
        printf("scene: chess-like frame + sampled hypotheses from files\n");
    }
    float *d_xyz, *d_staged, *d_err, *d_ref, *d_part, *d_md;
    double *d_soft, *d_soft_ref;
    CK(hipMalloc(&d_xyz, xyz.size() * 4)); CK(hipMalloc(&d_staged, staged.size() * 4));
    CK(hipMalloc(&d_err, (size_t)N * P * 4)); CK(hipMalloc(&d_ref, (size_t)N * P * 4));
    CK(hipMalloc(&d_part, (size_t)dk::reproject_num_pixel_tiles(P) * N * 4)); CK(hipMalloc(&d_md, 4));
    CK(hipMalloc(&d_soft, (size_t)N * 8)); CK(hipMalloc(&d_soft_ref, (size_t)N * 8));
    CK(hipMemcpy(d_xyz, xyz.data(), xyz.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_staged, staged.data(), staged.size() * 4, hipMemcpyHostToDevice));
    dk::FrameDev F{};
    F.xyz = d_xyz; F.uv = nullptr; F.H = H; F.W = W; F.P = P; F.fx = F.fy = 525.f; F.cx = 320.f; F.cy = 240.f;
    F.frames = frames; F.xyz_stride = (long long)P * 3; F.uv_stride = 0;
    hipStream_t st; CK(hipStreamCreate(&st));
    hipEvent_t ea, eb; CK(hipEventCreate(&ea)); CK(hipEventCreate(&eb));
    hipEvent_t da = nullptr, db = nullptr;  // when set: timing events attached to the K2 dispatch itself, as dsac_profile_enable does
    auto run = [&](int variant, int flags, float* err, double* soft) {
        dk::K2PlanIn in;  // staged records only, no cv poses: the fp32 forms
        in.o.variant = variant; in.o.flags = flags; in.o.pixel_minor = true;
        if (flags & 64) { err = nullptr; in.o.flags &= ~64; }  // arithmetic only: soft sums without the error-image output
        in.N = N; in.Nf = frames > 1 ? Nf : 0; in.frames = frames; in.P = P; in.W = W; in.poses = false;
        in.want_err = err != nullptr; in.want_soft = true;
        const dk::K2Plan plan = dk::k2_plan(in);
        dk::K2Call call;
        call.ev_start = da; call.ev_stop = db;
        const int used = plan.tiles;
        hipError_t e = dk::reproject(st, plan, N, d_staged, F, 100.f, err, 10.f, 0.5f, d_part, call);
        if (e != hipSuccess) { printf("variant %d: %s\n", variant, hipGetErrorString(e)); exit(1); }
        if (soft) CK(dk::reduce_soft(st, N, used, d_part, soft));
    };
    // settle clocks: ~0.4 s of the default form
    for (int i = 0; i < 400; i++) run(21, 0, d_ref, nullptr);
    CK(hipStreamSynchronize(st));
    // reference: the round-2 default form
    run(21, 0, d_ref, d_soft_ref);
    CK(hipStreamSynchronize(st));
    std::vector<double> sref(N), s(N);
    CK(hipMemcpy(sref.data(), d_soft_ref, (size_t)N * 8, hipMemcpyDeviceToHost));
    printf("frames %d  N %d  P %d  volume %.2f GB ; soft[0..3] = %.3f %.3f %.3f %.3f\n", frames, N, P, (double)N * P * 4 / 1e9, sref[0], sref[1], sref[2], sref[3]);
    const double bytes = (double)frames * (12.0 * P + 48.0 * Nf + 4.0 * Nf * P + 4.0 * Nf);
    for (const std::string& vs : vars) {
        int variant = atoi(vs.c_str()), flags = 0;
        const size_t col = vs.find(':');
        if (col != std::string::npos) flags = atoi(vs.c_str() + col + 1);
        CK(hipMemsetAsync(d_err, 0, (size_t)N * P * 4, st));
        run(variant, flags, d_err, d_soft);
        CK(hipMemsetAsync(d_md, 0, 4, st));
        hipLaunchKernelGGL(k_maxdiff, dim3(4096), dim3(256), 0, st, d_err, d_ref, (size_t)N * P, d_md);
        float md; CK(hipMemcpyAsync(&md, d_md, 4, hipMemcpyDeviceToHost, st));
        CK(hipMemcpyAsync(s.data(), d_soft, (size_t)N * 8, hipMemcpyDeviceToHost, st));
        CK(hipStreamSynchronize(st));
        double mrel = 0;
        for (int h = 0; h < N; h++) mrel = fmax(mrel, fabs(s[h] - sref[h]) / fmax(1.0, fabs(sref[h])));
        for (int i = 0; i < 20; i++) run(variant, flags, d_err, nullptr);
        float best = 1e9f, sum = 0;
        const int reps = 4, per = 25;  // sustained: batches of back-to-back launches, no host synchronisation inside a batch
        for (int i = 0; i < reps; i++) {
            CK(hipEventRecord(ea, st));
            for (int k = 0; k < per; k++) run(variant, flags, d_err, nullptr);
            CK(hipEventRecord(eb, st));
            CK(hipEventSynchronize(eb));
            float ms; CK(hipEventElapsedTime(&ms, ea, eb));
            ms /= per;
            best = fminf(best, ms); sum += ms;
        }
        // the bench's way: events attached to each dispatch, launches back to back
        double dsum = 0;
        {
            const int nd = 20;
            std::vector<hipEvent_t> evs(2 * nd);
            for (auto& ev_ : evs) CK(hipEventCreate(&ev_));
            for (int k = 0; k < nd; k++) { da = evs[2 * k]; db = evs[2 * k + 1]; run(variant, flags, d_err, getenv("K2LAB_REDUCE") ? d_soft : nullptr); }
            da = db = nullptr;
            CK(hipStreamSynchronize(st));
            for (int k = 0; k < nd; k++) { float ms; CK(hipEventElapsedTime(&ms, evs[2 * k], evs[2 * k + 1])); dsum += ms; }
            for (auto& ev_ : evs) CK(hipEventDestroy(ev_));
            dsum /= nd;
        }
        printf("variant %-8s : mean %7.1f us  best %7.1f us  %6.0f GB/s (%.3f of 8 TB/s)   dispatch-timed %7.1f us   max|err - ref| %.3g   max rel soft diff %.3g\n", vs.c_str(), sum / reps * 1e3,
               best * 1e3, bytes / (sum / reps) / 1e6, bytes / (sum / reps) / 1e6 / 8000.0, dsum * 1e3, md, mrel);
        fflush(stdout);
    }
    return 0;
}
