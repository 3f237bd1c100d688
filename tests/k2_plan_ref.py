"""Which K2 kernel scores a frame: the policy restated in Python, for tests/test_k2_plan_cpu.py to hold dk::k2_plan (dsac_amd/csrc/k2_plan.h) against.

Written from the code the plan replaced -- the launch function dk::reproject() with its refusals, its auto policy and the row counts its launchers reported,
the records k2_stage() built in front of it, and k2_soft_part()'s prediction of the fused sums -- in the order that code took its decisions: one block per
early return.  It is array code (numpy) only so that the test's cross product of some twenty million cases takes seconds; `variant` is one id per call,
every other argument broadcasts.  Two things are deliberately not what that code did, both out of reach of the C ABI (dsac_set_option refuses ids it does
not know, the 16-bit entry points refuse every k2_variant but -1 by name):
  * need_split / need_lo are the records the chosen kernel READS; the old stage also built split records in front of a forced fp32 kernel, in front of the
    two-piece form, and in front of launches that were then refused
  * 16-bit error images with a k2_variant below -1 (only DSAC_K2_VARIANT can set one) are refused; the old backstop read `variant < 0` and would have let the
    float-storing build 84 write into the 16-bit buffer

`mutant` plants one one-line mistake (MUTANTS); the test asserts that each is noticed."""
import numpy as np

OK, INVALID, NOT_SUPPORTED = 0, 1, 801
F32, F16, BF16 = 0, 1, 2
STORE_ONLY, UNFUSED, PRECISE, REC32, RECLO, EXACT, EXACT_ANY = 1 << 1, 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 29
FORM_NONE, FORM_VALU, FORM_MFMA, FORM_RECLO, FORM_EXACT_VEC, FORM_EXACT_ANY, FORM_PRECISE = range(7)
WHY_AUTO_OFF, WHY_FORCED, WHY_FOCAL, WHY_NO_POSES = 1, 2, 4, 8
FAM_NONE, FAM_VALU_SCALAR, FAM_VALU, FAM_HP, FAM_ST, FAM_PS, FAM_RECLO, FAM_EXACT_VEC, FAM_EXACT_ANY, FAM_PRECISE = range(10)

FIELDS = ("status", "form", "why", "family", "id", "px", "ht", "ng", "ch", "wv", "pw", "minw", "exf", "need_split", "need_lo", "fuse_sums", "kflags",
          "pixel_minor", "Nf", "tiles")
MUTANTS = ("threshold_ge", "split_for_forced_fp32", "any_tail_row_forgotten", "f16_without_p8")

# the launch switch, case by case: (pixels per thread, hypotheses per workgroup) of the VALU kernels
VA = {0: (4, 32), 1: (4, 32), 2: (4, 16), 3: (4, 64), 10: (4, 1), 11: (4, 2), 12: (4, 4), 13: (4, 8)}
# (hypotheses per workgroup, 64-pixel chunks per wave) of the matrix-core kernels
HP = {20: (64, 2), 21: (64, 4), 22: (128, 2), 23: (32, 2), 24: (64, 1), 25: (128, 4), 26: (32, 4), 27: (128, 1)}
# (16-hypothesis groups, chunks per wave, waves per workgroup, per-wave sums, waves per SIMD) of the streaming kernels
ST = {40: (1, 1, 4, 0, 1), 41: (2, 1, 4, 0, 1), 42: (4, 1, 4, 0, 1), 43: (2, 2, 4, 0, 1), 44: (1, 4, 1, 1, 1), 45: (2, 4, 1, 1, 1), 46: (4, 4, 1, 1, 1),
      47: (1, 2, 1, 1, 1), 48: (2, 2, 1, 1, 1), 49: (4, 2, 1, 1, 1), 50: (1, 1, 1, 1, 1), 51: (2, 1, 1, 1, 1), 52: (4, 1, 1, 1, 1), 53: (2, 1, 4, 1, 1),
      54: (2, 2, 4, 1, 1), 55: (4, 1, 4, 1, 1), 56: (2, 4, 4, 1, 1), 57: (4, 2, 4, 1, 1), 58: (4, 4, 1, 1, 4), 59: (2, 4, 1, 1, 5), 65: (4, 4, 4, 1, 4),
      66: (4, 4, 2, 1, 4), 67: (1, 4, 4, 1, 1), 68: (2, 4, 4, 0, 1), 69: (2, 4, 8, 1, 1), 70: (2, 4, 4, 1, 4), 71: (1, 4, 8, 1, 1), 72: (2, 4, 16, 1, 1),
      73: (2, 8, 1, 1, 1), 74: (1, 8, 1, 1, 1), 75: (2, 6, 1, 1, 1), 76: (2, 3, 1, 1, 1), 77: (1, 6, 1, 1, 1)}
for _v in (80, 81, 82, 83, 84, 85, 89, 93, 94, 95):  # without their flag: the plain form 58
    ST[_v] = ST[58]
PS = {60: 1, 61: 2, 62: 4}  # 16-hypothesis groups of the persistent kernels, four waves per workgroup
LO = {80: (4, 4, 3), 81: (4, 4, 2), 82: (4, 2, 4), 83: (2, 4, 3)}  # two-piece records: (groups, chunks, waves per SIMD)
EX = {84: (4, 4, 2, 1), 85: (4, 4, 2, 2), 89: (2, 4, 2, 1), 93: (4, 1, 3, 1), 94: (4, 1, 3, 2), 95: (4, 1, 4, 2)}  # exact vector build: (.., .., .., tail)
KNOWN = sorted(set(VA) | set(HP) | set(ST) | set(PS))


def cdiv(a, b):
    return (a + b - 1) // b


def plan(variant, flags, exact_auto, pixel_minor, f16_store, N, Nf, frames, P, W, uv, xyz_al, uv_al, err_al, focal_ok, poses, want_err, want_soft, elem,
         mutant=None):
    assert mutant is None or mutant in MUTANTS
    variant = int(variant)
    args = np.broadcast_arrays(*[np.asarray(a, np.int32) for a in (flags, exact_auto, pixel_minor, f16_store, N, Nf, frames, P, W, uv, xyz_al, uv_al, err_al,
                                                                  focal_ok, poses, want_err, want_soft, elem)])
    flags, exact_auto, pixel_minor, f16_store, N, Nf, frames, P, W, uv, xyz_al, uv_al, err_al, focal_ok, poses, want_err, want_soft, elem = args
    b = lambda a: a != 0
    exact_auto, pixel_minor, uv, xyz_al, uv_al, err_al, focal_ok, poses, want_err, want_soft = map(
        b, (exact_auto, pixel_minor, uv, xyz_al, uv_al, err_al, focal_ok, poses, want_err, want_soft))
    out = {f: np.zeros(flags.shape, np.int32) for f in FIELDS}
    out["id"][:] = -1
    out["pixel_minor"][:] = 1
    live = np.ones(flags.shape, bool)

    def settle(m, **kw):
        """the cases of m that are still undecided end here with these fields"""
        nonlocal live
        m = live & m
        for f, v in kw.items():
            out[f][m] = v[m] if isinstance(v, np.ndarray) else v
        live = live & ~m

    bytes_ = N.astype(np.float64) * P.astype(np.float64) * 4.0
    over = (lambda x, t: x >= t) if mutant == "threshold_ge" else (lambda x, t: x > t)
    # k2_soft_part: an error-images-only call on a big launch gets the buffer for the sums all the same
    fused = ~want_soft & want_err & (variant < 0) & ~b(flags & UNFUSED) & over(bytes_, 1.0e9)
    err, soft = want_err, want_soft | fused
    # reproject(): nothing to do
    settle((N <= 0) | (P <= 0) | (~err & ~soft))
    one = (Nf <= 0) | (frames <= 1)
    settle(~one & (Nf % 128 != 0), status=INVALID)
    Nf_k = np.where(one, cdiv(N, 128) * 128, Nf)
    vec = (P % 4 == 0) & err_al & xyz_al & uv_al
    kf = flags | np.where((variant >= 40) & ~pixel_minor, 32, 0)
    wants_exact = b(flags & (EXACT | EXACT_ANY)) | (exact_auto & (variant < 0) & ~b(flags & (PRECISE | RECLO | STORE_ONLY | REC32)))
    # k2_stage: the records it built and handed over
    split = poses & wants_exact & focal_ok
    lo = poses & b(flags & RECLO)
    split_ok = split & focal_ok
    ex_variant = variant in EX
    why = np.zeros(flags.shape, np.int32)
    no_ex_bit = ~b(flags & (EXACT | EXACT_ANY))
    forced = (variant >= 0) | b(flags & (PRECISE | RECLO | STORE_ONLY | REC32))
    why |= np.where(no_ex_bit & forced, WHY_FORCED, 0)
    why |= np.where(no_ex_bit & ~forced & ~exact_auto, WHY_AUTO_OFF, 0)
    why |= np.where(~no_ex_bit & (variant >= 0) & (not ex_variant), WHY_FORCED, 0)
    why |= np.where(~focal_ok, WHY_FOCAL, 0)
    why |= np.where(~poses, WHY_NO_POSES, 0)
    # 16-bit error images: the auto policy's exact vector build or an error (see the note on ids below -1 above: the old code read variant < 0)
    p8 = True if mutant == "f16_without_p8" else (P % 8 == 0)
    settle((elem != F32) & ~(err & vec & p8 & split_ok & (variant == -1) & wants_exact & ~b(flags & ~(EXACT | EXACT_ANY))), status=NOT_SUPPORTED)
    # a form that was asked for and cannot run on this map
    prec_map = vec & (uv | (W % 4 == 0))
    settle(poses & ((b(flags & PRECISE) & ~prec_map) | (b(flags & RECLO) & ~vec) | (b(flags & EXACT) & ~(vec & split_ok)) |
                    (b(flags & EXACT_ANY) & ~(split_ok & ((variant < 0) | (ex_variant & vec))))), status=NOT_SUPPORTED)
    settle(b(flags & EXACT_ANY) & ~poses, status=NOT_SUPPORTED)
    common = dict(fuse_sums=fused.astype(np.int32), Nf=Nf_k, pixel_minor=pixel_minor.astype(np.int32))
    # what the old stage built and what the kernel reads are not the same thing: see the module's note
    ns = lambda reads: (split if mutant == "split_for_forced_fp32" else (split & reads)).astype(np.int32)
    yes, no = np.ones(flags.shape, bool), np.zeros(flags.shape, bool)
    # the precise form
    settle(b(flags & PRECISE) & poses & prec_map, form=FORM_PRECISE, why=why, family=FAM_PRECISE, ht=np.where(N.astype(np.float64) * P > 2.0e8, 32, 16),
           kflags=kf, tiles=2 * cdiv(P, 1024), need_split=ns(no), **common)
    # records in two pieces
    if variant < 0 or variant in LO:
        ng, ch, mw = LO[variant if variant in LO else 81]
        settle(b(flags & RECLO) & lo & vec, form=FORM_RECLO, why=why, family=FAM_RECLO, id=variant if variant in LO else 81, ng=ng, ch=ch, wv=1, pw=1, minw=mw,
               kflags=kf | 32, tiles=cdiv(P, ch * 64), need_lo=1, need_split=ns(no), **common)
    # the exact form, any-map build: the policy's tile for the map's size, one more row for the tail launch
    if variant < 0:
        small = P <= 16384
        ch = np.where(small, 1, 4)
        tail = 0 if mutant == "any_tail_row_forgotten" else np.where((P % 4 != 0) & soft, 1, 0)
        settle(wants_exact & split_ok & ~vec, form=FORM_EXACT_ANY, why=0, family=FAM_EXACT_ANY, id=-1, ng=4, ch=ch, wv=1, pw=1, minw=np.where(small, 3, 2), exf=2,
               kflags=kf | 32, tiles=cdiv(P, ch * 64) + tail, need_split=ns(yes), **common)
    # the exact form, vector build
    if variant < 0 or ex_variant:
        if variant == -1:
            small = P <= 16384
            ng, ch, mw = 4, np.where(small, 1, 4), np.where(small, 3, 2)
            exf = np.where(elem == F16, np.where(f16_store == 0, 3, 4), np.where(elem == BF16, np.where(f16_store == 0, 5, 6), 2))
            kid = -1
        else:
            kid = variant if ex_variant else 84  # the switch's default
            ng, ch, mw, exf = EX[kid]
        settle(wants_exact & split_ok & vec, form=FORM_EXACT_VEC, why=0, family=FAM_EXACT_VEC, id=kid, ng=ng, ch=ch, wv=1, pw=1, minw=mw, exf=exf, kflags=kf | 32,
               tiles=cdiv(P, ch * 64), need_split=ns(yes), **common)
    # the fp32 forms.  A map the vector kernels cannot read: one pixel per thread, whatever the id
    settle(~vec, form=FORM_VALU, why=why, family=FAM_VALU_SCALAR, kflags=kf, tiles=cdiv(P, 256), need_split=ns(no), **common)
    if variant < 0:
        big = over(bytes_, 1.0e9)
        grid64 = ~uv & (W & 63 == 0)
        ids = np.where(soft, np.where(big, np.where(grid64 & over(bytes_, 4.4e9), 58, 45), 42), 0)
        kf = kf | np.where(soft & big, 32, 0)
        common["pixel_minor"] = 1
        form = np.where(soft, FORM_MFMA, FORM_VALU)
    else:
        ids = np.full(flags.shape, variant)
        form = FORM_VALU if variant <= 13 else FORM_MFMA
    for kid in np.unique(ids[live]):
        kid = int(kid)
        m = ids == kid
        if kid in VA:
            settle(m, form=form, why=why, family=FAM_VALU, id=kid, px=VA[kid][0], ht=VA[kid][1], kflags=kf, tiles=cdiv(P, 256 * VA[kid][0]), need_split=ns(no), **common)
        elif kid in HP:
            settle(m, form=form, why=why, family=FAM_HP, id=kid, ht=HP[kid][0], ch=HP[kid][1], kflags=kf, tiles=cdiv(P, 256 * HP[kid][1]), need_split=ns(no), **common)
        elif kid in ST:
            ng, ch, wv, pw, mw = ST[kid]
            PT = cdiv(P, wv * ch * 64)
            settle(m, form=form, why=why, family=FAM_ST, id=kid, ng=ng, ch=ch, wv=wv, pw=pw, minw=mw, kflags=kf, tiles=PT * wv if pw else PT, need_split=ns(no),
                   **common)
        elif kid in PS:
            settle(m & (N % 4 != 0) & soft, status=INVALID)  # the sums leave as 16-byte stores
            settle(m, form=form, why=why, family=FAM_PS, id=kid, ng=PS[kid], wv=4, kflags=kf, tiles=cdiv(P, 64), need_split=ns(no), **common)
        else:
            settle(m, status=INVALID)  # no such kernel
    assert not live.any()
    return out


def known(variant):
    """reproject_variant_known()"""
    v = variant
    return v == -1 or 0 <= v <= 3 or 10 <= v <= 13 or 20 <= v <= 27 or 40 <= v <= 62 or 65 <= v <= 77 or 80 <= v <= 85 or v == 89 or 93 <= v <= 95


def num_pixel_tiles(P):
    """reproject_num_pixel_tiles(): the rows soft_part is sized for"""
    return (P + 63) // 64 + 15
