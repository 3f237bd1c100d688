// Test harness (tests/test_k2_plan_cpu.py): dsac_amd/csrc/k2_plan.h compiled for the host by a plain C++ compiler.  Plans travel as rows of ints.
#include "../../dsac_amd/csrc/k2_plan.h"
#include <cstdint>

extern "C" {

// in: n rows of {variant, flags, exact_auto, pixel_minor, f16_store, N, Nf, frames, P, W, uv, xyz_al16, uv_al16, err_al16, focal_ok, poses, want_err,
// want_soft, err_elem};  out: n rows of {status, form, why, family, id, px, ht, ng, ch, wv, pw, minw, exf, need_split, need_lo, fuse_sums, kflags,
// pixel_minor, Nf, tiles}
enum { K2P_IN = 19, K2P_OUT = 20 };
int k2p_in_fields() { return K2P_IN; }
int k2p_out_fields() { return K2P_OUT; }
void k2p_plan(int64_t n, const int32_t* in, int32_t* out) {
    for (int64_t i = 0; i < n; i++) {
        const int32_t* a = in + i * K2P_IN;
        dk::K2PlanIn q;
        q.o.variant = a[0]; q.o.flags = a[1]; q.o.exact_auto = a[2] != 0; q.o.pixel_minor = a[3] != 0; q.o.f16_store = a[4];
        q.N = a[5]; q.Nf = a[6]; q.frames = a[7]; q.P = a[8]; q.W = a[9]; q.uv = a[10] != 0;
        q.xyz_al16 = a[11] != 0; q.uv_al16 = a[12] != 0; q.err_al16 = a[13] != 0;
        q.focal_ok = a[14] != 0; q.poses = a[15] != 0; q.want_err = a[16] != 0; q.want_soft = a[17] != 0; q.err_elem = a[18];
        const dk::K2Plan p = dk::k2_plan(q);
        const int32_t r[K2P_OUT] = {p.status, p.form, p.why, p.k.family, p.k.id, p.k.px, p.k.ht, p.k.ng, p.k.ch, p.k.wv, p.k.pw, p.k.minw, p.k.exf,
                                    p.need_split, p.need_lo, p.fuse_sums, p.kflags, p.pixel_minor, p.Nf, p.tiles};
        for (int k = 0; k < K2P_OUT; k++) out[i * K2P_OUT + k] = r[k];
    }
}
int k2p_variant_known(int v) { return dk::k2_variant_known(v) ? 1 : 0; }
int k2p_num_pixel_tiles(int P) { return dk::reproject_num_pixel_tiles(P); }
int k2p_exact_only(int variant, int flags, int exact_auto) { return dk::k2_exact_only(variant, flags, exact_auto != 0); }
int k2p_fuse_sums(int variant, int flags, int N, int P, int want_err, int want_soft) {
    dk::K2Opts o;
    o.variant = variant; o.flags = flags;
    return dk::k2_fuse_sums(o, N, P, want_err != 0, want_soft != 0) ? 1 : 0;
}
}
