// Test harness (tests/test_k2_walk_plan_cpu.py): the hypothesis walk of dsac_amd/csrc/k2_plan.h compiled for the host by a plain C++ compiler.
#include "../../dsac_amd/csrc/k2_plan.h"
#include <cstdint>

extern "C" {

// in: n rows of k2_plan_host.cpp's 19 inputs + {hyp_walk option};  out: n rows of its 20 outputs + {hyp_walk, walks}: `walks` is the hypothesis dimension of
// the grid the launch builds for a streaming kernel (k2_walks), 0 for the other families
enum { K2W_IN = 20, K2W_OUT = 22 };
int k2w_in_fields() { return K2W_IN; }
int k2w_out_fields() { return K2W_OUT; }
void k2w_plan(int64_t n, const int32_t* in, int32_t* out) {
    for (int64_t i = 0; i < n; i++) {
        const int32_t* a = in + i * K2W_IN;
        dk::K2PlanIn q;
        q.o.variant = a[0]; q.o.flags = a[1]; q.o.exact_auto = a[2] != 0; q.o.pixel_minor = a[3] != 0; q.o.f16_store = a[4];
        q.N = a[5]; q.Nf = a[6]; q.frames = a[7]; q.P = a[8]; q.W = a[9]; q.uv = a[10] != 0;
        q.xyz_al16 = a[11] != 0; q.uv_al16 = a[12] != 0; q.err_al16 = a[13] != 0;
        q.focal_ok = a[14] != 0; q.poses = a[15] != 0; q.want_err = a[16] != 0; q.want_soft = a[17] != 0; q.err_elem = a[18];
        q.o.hyp_walk = a[19];
        const dk::K2Plan p = dk::k2_plan(q);
        const int walks = p.k.ng > 0 ? dk::k2_walks(q.N, p.k.ng, p.hyp_walk) : 0;
        const int32_t r[K2W_OUT] = {p.status, p.form, p.why, p.k.family, p.k.id, p.k.px, p.k.ht, p.k.ng, p.k.ch, p.k.wv, p.k.pw, p.k.minw, p.k.exf,
                                    p.need_split, p.need_lo, p.fuse_sums, p.kflags, p.pixel_minor, p.Nf, p.tiles, p.hyp_walk, walks};
        for (int k = 0; k < K2W_OUT; k++) out[i * K2W_OUT + k] = r[k];
    }
}
int k2w_auto_walk() { return dk::K2_WALK_AUTO; }
}
