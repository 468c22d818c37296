// fd_train_bwd_impl.h -- host side of fd_train_backward, fd_l1_loss, fd_sgd_step and the library-issued gradient exchange (translation unit fd_train_bwd.hip)
#pragma once
#include "fd_train_plan.h"

namespace {

struct BwdCtx {
    fd_train_plan *p;
    const fd_layer_params *params;
    const fd_layer_grads *grads;
    hipStream_t s;
    // weight-gradient partials of the units processed so far in this range: reduced by ONE launch at the end of the range
    // (fd_reduce_weights_batch_f32)
    fd_wbatch wb{};
};

int flush_weights(BwdCtx &c)
{
    if (!c.wb.count) return FD_OK;
    FD_LAUNCH(fd_reduce_weights_batch_f32, dim3((unsigned)c.wb.cb_start[c.wb.count]), dim3(1024), 0, c.s, c.wb);
    c.wb.count = 0;
    return check_launch("fd_reduce_weights_batch_f32");
}
int defer_weights(BwdCtx &c, const float *part, int nrows, int n, int KK, int C, float *out)
{
    if (n % 4) return fail(FD_ERR_INVALID, "weight tensor of %d elements: the batched reduction needs a multiple of 4", n);
    if (c.wb.count == FD_WBATCH_MAX) { int rc = flush_weights(c); if (rc) return rc; }
    if (c.wb.count == 0) c.wb.cb_start[0] = 0;
    c.wb.e[c.wb.count] = fd_wred_args{part, out, nrows, n, KK, C};
    c.wb.cb_start[c.wb.count + 1] = c.wb.cb_start[c.wb.count] + ceil_div(n, nrows <= FD_WBATCH_FEW_ROWS ? 4096 : 64);
    ++c.wb.count;
    return FD_OK;
}

inline fd_bn_bwd_fin bwd_fin_args(BwdCtx &c, int i, size_t cf_off)
{
    TLayer &L = c.p->layers[i];
    return fd_bn_bwd_fin{stat_ptr(c.p, L.sb_off), L.nr_b, stat_pitch(L.d.cout), (int)cf_off, 1.0 / L.n_stat, tws(c.p, L.st_off), c.grads[i].bn_weight, c.grads[i].bn_bias, tws(c.p, L.coef_off)};
}
int bn_bwd_finalize(BwdCtx &c, int i)
{
    TLayer &L = c.p->layers[i];
    const fd_bn_bwd_fin fa = bwd_fin_args(c, i, 0);
    FD_LAUNCH(fd_bn_bwd_finalize_rows_f32, dim3((unsigned)ceil_div(L.d.cout, 16)), dim3(256), 0, c.s, fa, L.d.cout);
    return check_launch("fd_bn_bwd_finalize_rows_f32");
}
// unit u's statistics rows are complete (its consumer's backward kernels have been launched): unless u's first backward kernel finalises them itself
// (TLayer::bwd_fin_rows), the separate launch
int finalize_or_defer(BwdCtx &c, int u) { return c.p->layers[u].bwd_fin_rows ? FD_OK : bn_bwd_finalize(c, u); }
// depthwise unit i's weight-gradient partial rows (one per row of its plan-sized region) go to the batched reduction
int defer_dw_weights(BwdCtx &c, int i)
{
    const TLayer &L = c.p->layers[i];
    const int kk = L.d.ksize * L.d.ksize;
    return defer_weights(c, tws(c.p, L.wp_off), (int)(L.wp_elems / ((size_t)kk * L.d.cin)), kk * L.d.cin, kk, L.d.cin, c.grads[i].conv_weight);
}

// ---- depthwise backward, one launcher per form (TLayer::DwBwd, chosen and sized by fd_train_plan_create) ----
template <typename T, int K, int S, int MODE, int ACT_IN, int ADD_SG>
int launch_dw_dgrad(BwdCtx &c, int i)
{
    TLayer &L = c.p->layers[i];
    TLayer &P = c.p->layers[L.d.src];
    const TLayer *Kp = L.d.skip >= 0 ? &c.p->layers[L.d.skip] : nullptr;
    const dim3 grid(L.d_gx, ceil_div(L.d.cin, L.dw_n << L.cbq), c.p->B);
    fd_by_lane_width<T>(L.dw_n, [&](auto nt) {
        constexpr int NL = decltype(nt)::value;
        if (L.blds2 > 64 * 1024) (void)hipFuncSetAttribute((const void *)fd_dw_dgrad<T, K, S, MODE, ACT_IN, ADD_SG, NL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.blds2);
        FD_LAUNCH((fd_dw_dgrad<T, K, S, MODE, ACT_IN, ADD_SG, NL>), grid, dim3(256), L.blds2, c.s, twt<T>(c.p, L.g_off), twt<T>(c.p, L.z_off), tws(c.p, L.coef_off),
                  c.params[i].conv_weight, twt<T>(c.p, P.z_off), tws(c.p, P.st_off), ADD_SG ? twt<T>(c.p, P.sg_off) : (const T *)nullptr,
                  twt<T>(c.p, P.g_off), Kp ? twt<T>(c.p, Kp->sg_off) : (T *)nullptr, bwd_rows(c.p, L.d.src),
                  L.in_h, L.in_w, L.out_h, L.out_w, L.d.cin, L.cbq, L.d_th, L.d_tw, L.d_tiles_x, L.csplit, L.bpstr);
    });
    return check_launch("fd_dw_dgrad");
}

template <typename T, int ACT_IN, int ADD_SG>
int dispatch_dw_dgrad(BwdCtx &c, int i)
{
    const TLayer &L = c.p->layers[i];
    const int key = L.d.ksize * 100 + L.d.stride * 10 + L.mode;
    switch (key) {
    case 310: return launch_dw_dgrad<T, 3, 1, 0, ACT_IN, ADD_SG>(c, i);
    case 320: return launch_dw_dgrad<T, 3, 2, 0, ACT_IN, ADD_SG>(c, i);
    case 510: return launch_dw_dgrad<T, 5, 1, 0, ACT_IN, ADD_SG>(c, i);
    case 511: return launch_dw_dgrad<T, 5, 1, 1, ACT_IN, ADD_SG>(c, i);
    case 512: return launch_dw_dgrad<T, 5, 1, 2, ACT_IN, ADD_SG>(c, i);
    case 513: return launch_dw_dgrad<T, 5, 1, 3, ACT_IN, ADD_SG>(c, i);
    }
    return fail(FD_ERR_INVALID, "train: depthwise backward k=%d stride=%d mode=%d has no kernel", L.d.ksize, L.d.stride, L.mode);
}

template <typename T, int ACT1, int ACT2>
int launch_dw_wgrad_acts(BwdCtx &c, int i)
{
    TLayer &L = c.p->layers[i];
    TLayer &P = c.p->layers[L.d.src];
    const TLayer *Kp = L.d.skip >= 0 ? &c.p->layers[L.d.skip] : nullptr;
    const int key = L.d.ksize * 100 + L.d.stride * 10 + L.mode;
    const dim3 wgrid(L.w_gx, ceil_div(L.d.cin, L.dw_n << L.cbq), c.p->B);
#define FD_DWW(K_, S_, M_)                                                                                                         \
    case K_ * 100 + S_ * 10 + M_:                                                                                                  \
        fd_by_lane_width<T>(L.dw_n, [&](auto nt) {                                                                                \
            constexpr int NL = decltype(nt)::value;                                                                               \
            FD_LAUNCH((fd_dw_wgrad<T, K_, S_, M_, ACT1, ACT2, NL>), wgrid, dim3(256), L.blds, c.s, twt<T>(c.p, P.z_off), tws(c.p, P.st_off),  \
                      Kp ? twt<T>(c.p, Kp->z_off) : (const T *)nullptr, Kp ? tws(c.p, Kp->st_off) : (const float *)nullptr,           \
                      twt<T>(c.p, L.g_off), twt<T>(c.p, L.z_off), tws(c.p, L.coef_off), tws(c.p, L.wp_off), L.in_h, L.in_w, L.out_h, L.out_w, L.d.cin, \
                      L.cbq, L.bth, L.btw, L.w_tiles_x, L.w_tpw, L.csplit, L.bpstr);                                              \
        });                                                                                                                        \
        break;
    switch (key) {
        FD_DWW(3, 1, 0) FD_DWW(3, 2, 0) FD_DWW(5, 1, 0) FD_DWW(5, 1, 1) FD_DWW(5, 1, 2) FD_DWW(5, 1, 3)
    default: return fail(FD_ERR_INVALID, "train: depthwise wgrad has no kernel for this layer");
    }
#undef FD_DWW
    return check_launch("fd_dw_wgrad");
}

// SEPARATE: the two kernels one after the other (every activation / composition has an instance)
template <typename T>
int launch_dw_separate(BwdCtx &c, int i)
{
    const TLayer &L = c.p->layers[i];
    const TLayer &P = c.p->layers[L.d.src];
    const int a1 = P.d.act, a2 = L.d.skip >= 0 ? c.p->layers[L.d.skip].d.act : FD_ACT_RELU6;
    int rc;
    if (a1 == FD_ACT_RELU6 && a2 == FD_ACT_RELU6) rc = launch_dw_wgrad_acts<T, FD_ACT_RELU6_, FD_ACT_RELU6_>(c, i);
    else if (a1 == FD_ACT_RELU && a2 == FD_ACT_RELU6) rc = launch_dw_wgrad_acts<T, FD_ACT_RELU_, FD_ACT_RELU6_>(c, i);
    else if (a1 == FD_ACT_RELU && a2 == FD_ACT_RELU) rc = launch_dw_wgrad_acts<T, FD_ACT_RELU_, FD_ACT_RELU_>(c, i);
    else rc = launch_dw_wgrad_acts<T, FD_ACT_RELU6_, FD_ACT_RELU_>(c, i);
    if (rc || (rc = defer_dw_weights(c, i))) return rc;
    const bool add = P.skip_consumer >= 0 && L.mode == 0;
    if (a1 == FD_ACT_RELU6) return add ? dispatch_dw_dgrad<T, FD_ACT_RELU6_, 1>(c, i) : dispatch_dw_dgrad<T, FD_ACT_RELU6_, 0>(c, i);
    return add ? dispatch_dw_dgrad<T, FD_ACT_RELU_, 1>(c, i) : dispatch_dw_dgrad<T, FD_ACT_RELU_, 0>(c, i);
}

// the operands of unit i's backward and the LDS-tiled geometry (fd_dw_bwd_args: every other form copies its operands from here)
template <typename T, int ADD_SG>
fd_dw_bwd_args<T> dw_bwd_args(BwdCtx &c, int i)
{
    const TLayer &L = c.p->layers[i];
    const TLayer &P = c.p->layers[L.d.src];
    const TLayer *Kp = L.d.skip >= 0 ? &c.p->layers[L.d.skip] : nullptr;
    fd_dw_bwd_args<T> a{};
    a.G = twt<T>(c.p, L.g_off); a.Z = twt<T>(c.p, L.z_off); a.Zin = twt<T>(c.p, P.z_off);
    a.Zskip = Kp ? twt<T>(c.p, Kp->z_off) : nullptr; a.SG = ADD_SG ? twt<T>(c.p, P.sg_off) : nullptr;
    a.Gin = twt<T>(c.p, P.g_off); a.SGout = Kp ? twt<T>(c.p, Kp->sg_off) : nullptr;
    a.coef = tws(c.p, L.coef_off); a.w = c.params[i].conv_weight; a.st_in = tws(c.p, P.st_off); a.st_skip = Kp ? tws(c.p, Kp->st_off) : nullptr;
    a.sr = bwd_rows(c.p, L.d.src);
    a.wpart = tws(c.p, L.wp_off);
    a.Hin = L.in_h; a.Win = L.in_w; a.Ho = L.out_h; a.Wo = L.out_w; a.C = L.d.cin; a.cbq = L.cbq; a.csplit = L.csplit; a.pstr = L.bpstr; a.B = c.p->B;
    a.d_th = L.d_th; a.d_tw = L.d_tw; a.d_tiles_x = L.d_tiles_x; a.d_gx = L.d_gx; a.d_gy = ceil_div(L.d.cin, L.dw_n << L.cbq);
    a.w_th = L.bth; a.w_tw = L.btw; a.w_tiles_x = L.w_tiles_x; a.w_tpw = L.w_tpw; a.w_gx = L.w_gx; a.w_gy = a.d_gy;
    if (L.bwd_fin_rows && (L.bwd == TLayer::DwBwd::BWD1 || L.bwd == TLayer::DwBwd::PAIR))
        a.fin = bwd_fin_args(c, i, L.blds - (size_t)4 * (L.dw_n << L.cbq) * 4);       // (the coefficient block ends their LDS)
    return a;
}

// the forms with a kernel instance per (kernel size, stride, input composition, activations): fd_by_dw_instance
template <typename T, int K, int S, int MODE, int ACT1, int ACT2, int ADD_SG>
int launch_dw_form(BwdCtx &c, int i)
{
    using F = TLayer::DwBwd;
    constexpr bool H16 = !std::is_same<T, float>::value;
    const TLayer &L = c.p->layers[i];
    const fd_dw_bwd_args<T> a = dw_bwd_args<T, ADD_SG>(c, i);
    const unsigned B = (unsigned)c.p->B;
    switch (L.bwd) {
    case F::ROWS5:                                            // dz and the re-created input rounded to the storage type; the backward-data taps too
        if constexpr (H16 && K == 5 && S == 1 && MODE == 2 && !ADD_SG) {
            const fd_dw5_bwd_args<T> b{a.G, a.Z, a.Zin, a.Zskip, a.Gin, a.SGout, a.coef, a.w, a.st_in, a.st_skip, a.sr, a.wpart,
                                       L.in_h, L.in_w, L.d.cin, L.rb_groups, L.rb_bh, L.rb_bh, L.rb_wgs, L.rb_wgs, L.bwd_fin_rows ? bwd_fin_args(c, i, 0) : fd_bn_bwd_fin{}};
            FD_LAUNCH((fd_dw5_bwd_rows<T, ACT1, ACT2>), dim3((unsigned)(2 * L.rb_wgs), (unsigned)ceil_div(L.d.cin, 64), B), dim3(256), 0, c.s, b);
            return check_launch("fd_dw5_bwd_rows");
        }
        break;
    case F::ROWS3:                                            // (nothing rounded)
        if constexpr (H16 && K == 3 && S == 1 && MODE == 0 && !ADD_SG) {
            const fd_dw3_bwd_args<T> b{a.G, a.Z, a.Zin, a.Gin, a.coef, a.w, a.st_in, a.sr, a.wpart, L.in_h, L.in_w, L.d.cin, L.rb_groups, L.rb_bh, L.rb_bh, L.rb_wgs, L.rb_wgs,
                                       L.bwd_fin_rows ? bwd_fin_args(c, i, 0) : fd_bn_bwd_fin{}};
            const dim3 g3((unsigned)(2 * L.rb_wgs), (unsigned)ceil_div(L.d.cin, 2 * L.rb_cl), B);
            if (L.rb_cl == 16) FD_LAUNCH((fd_dw3_bwd_rows<T, ACT1, 16>), g3, dim3(256), 0, c.s, b);
            else FD_LAUNCH((fd_dw3_bwd_rows<T, ACT1, 32>), g3, dim3(256), 0, c.s, b);
            return check_launch("fd_dw3_bwd_rows");
        }
        break;
    case F::ROWS3S2:
        if constexpr (H16 && K == 3 && S == 2 && MODE == 0) {
            const fd_dw3s2_bwd_args<T> b{a.G, a.Z, a.Zin, a.SG, a.Gin, a.coef, a.w, a.st_in, a.sr, a.wpart, L.out_h, L.out_w, L.d.cin, L.rb_groups, L.rb_bh, L.rb_wgs,
                                         L.bwd_fin_rows ? bwd_fin_args(c, i, 0) : fd_bn_bwd_fin{}};
            FD_LAUNCH((fd_dw3s2_bwd_rows<T, ACT1, ADD_SG>), dim3((unsigned)L.rb_wgs, (unsigned)ceil_div(L.d.cin, 64), B), dim3(256), 0, c.s, b);
            return check_launch("fd_dw3s2_bwd_rows");
        }
        break;
    case F::REGWIN_S2:
        if constexpr (K == 3 && S == 2 && MODE == 0) {
            FD_LAUNCH((fd_dw3s2_dgrad_rows<T, ACT1, ADD_SG>), L.rw_grid_d, dim3(256), 0, c.s, a.G, a.Z, a.coef, a.w, a.Zin, a.st_in, a.SG, a.Gin, a.sr,
                      L.in_h, L.in_w, L.out_h, L.out_w, L.d.cin, L.rw_th_d);
            const int rc = check_launch("fd_dw3s2_dgrad_rows");
            if (rc) return rc;
            FD_LAUNCH((fd_dw3_wgrad_rows<T, 2, ACT1>), L.rw_grid_w, dim3(256), 0, c.s, a.Zin, a.st_in, a.G, a.Z, a.coef, a.wpart, L.in_h, L.in_w, L.out_h, L.out_w, L.d.cin, L.rw_th_w);
            return check_launch("fd_dw3_wgrad_rows");
        }
        break;
    case F::BWD1:                                             // (the instance with the in-kernel finalisation costs registers: only where it replaces a launch)
        fd_by_lane_width<T>(L.dw_n, [&](auto nt) {
            constexpr int NL = decltype(nt)::value;
            const dim3 grid((unsigned)a.d_gx, (unsigned)a.d_gy, B);
            if (a.fin.rows) {
                (void)hipFuncSetAttribute((const void *)fd_dw_bwd1<T, K, S, MODE, ACT1, ACT2, ADD_SG, NL, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.blds);
                FD_LAUNCH((fd_dw_bwd1<T, K, S, MODE, ACT1, ACT2, ADD_SG, NL, true>), grid, dim3(256), L.blds, c.s, a);
            } else {
                (void)hipFuncSetAttribute((const void *)fd_dw_bwd1<T, K, S, MODE, ACT1, ACT2, ADD_SG, NL, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.blds);
                FD_LAUNCH((fd_dw_bwd1<T, K, S, MODE, ACT1, ACT2, ADD_SG, NL, false>), grid, dim3(256), L.blds, c.s, a);
            }
        });
        return check_launch("fd_dw_bwd1");
    case F::PAIR:                                             // both roles in one launch
        fd_by_lane_width<T>(L.dw_n, [&](auto nt) {
            constexpr int NL = decltype(nt)::value;
            const dim3 grid((unsigned)(B * ((long)a.d_gx * a.d_gy + (long)a.w_gx * a.w_gy)));
            if (a.fin.rows) {
                if (L.blds > 64 * 1024) (void)hipFuncSetAttribute((const void *)fd_dw_bwd<T, K, S, MODE, ACT1, ACT2, ADD_SG, NL, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.blds);
                FD_LAUNCH((fd_dw_bwd<T, K, S, MODE, ACT1, ACT2, ADD_SG, NL, true>), grid, dim3(256), L.blds, c.s, a);
            } else {
                if (L.blds > 64 * 1024) (void)hipFuncSetAttribute((const void *)fd_dw_bwd<T, K, S, MODE, ACT1, ACT2, ADD_SG, NL, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.blds);
                FD_LAUNCH((fd_dw_bwd<T, K, S, MODE, ACT1, ACT2, ADD_SG, NL, false>), grid, dim3(256), L.blds, c.s, a);
            }
        });
        return check_launch("fd_dw_bwd");
    case F::SEPARATE: break;
    }
    return fail(FD_ERR_STATE, "train: depthwise unit %d has no instance of its backward form %d", i, (int)L.bwd);
}

template <typename T>
int launch_dw_bwd(BwdCtx &c, int i)
{
    if (c.p->layers[i].bwd == TLayer::DwBwd::SEPARATE) return launch_dw_separate<T>(c, i);
    int rc = FD_ERR_STATE;
    fd_by_dw_instance(c.p, i, [&](auto in) {
        using I = decltype(in);
        rc = launch_dw_form<T, I::K, I::S, I::MODE, I::ACT1, I::ACT2, I::ADD_SG>(c, i);
    });
    return rc ? rc : defer_dw_weights(c, i);
}

template <typename T, int ACT_IN>
int launch_pw_bwd_h16(BwdCtx &c, int i)
{
    TLayer &L = c.p->layers[i];
    TLayer &P = c.p->layers[L.d.src];
    const int M = (int)L.M, N = L.d.cout, K = L.d.cin;
    const T *Gsrc = twt<T>(c.p, L.g_off);
    T *G = L.dz_off ? twt<T>(c.p, L.dz_off) : twt<T>(c.p, L.g_off);     // dz: the operand of both GEMMs below
    int rc;
    // dz = BatchNorm-backward(G, z), in place over G: the operand of both GEMMs below
    {
        const long chunks = (long)M * N / 8;
        if (L.bwd_fin_rows) {                                 // the apply pass finalises the unit's BatchNorm backward itself
            const int gx = ceil_div(N, 64), gy = std::max(1, std::min(ceil_div(M, 32), 1024 / gx));
            const fd_bn_bwd_fin fa = bwd_fin_args(c, i, 0);
            FD_LAUNCH((fd_bn_bwd_apply_fin_h16<T>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, c.s, Gsrc, G, twt<T>(c.p, L.z_off), M, N, fa);
            if ((rc = check_launch("fd_bn_bwd_apply_fin_h16"))) return rc;
        } else {
            FD_LAUNCH((fd_bn_bwd_apply_h16<T>), dim3((unsigned)std::min<long>(4096, ceil_div(chunks, 256))), dim3(256), 0, c.s, Gsrc, G, twt<T>(c.p, L.z_off), tws(c.p, L.coef_off), chunks, N);
            if ((rc = check_launch("fd_bn_bwd_apply_h16"))) return rc;
        }
    }
    // weight gradient: output tiles x pixel splits
    const int n_tiles = ceil_div(N, 64), k_tiles_w = ceil_div(K, 64);
    int splits = std::max(1, std::min(ceil_div(FD_WGRAD_TARGET_WGS_H16, (long)n_tiles * k_tiles_w), ceil_div(M, 256)));
    const int rows = ceil_div(ceil_div(M, splits), 64) * 64;
    splits = ceil_div(M, rows);
    if ((size_t)splits * N * K > L.wp_elems) return fail(FD_ERR_STATE, "weight-gradient partial region too small");
    // backward data: 64 x 128 tiles of G_in when there are >= 128 input channels and that still leaves >= 200 workgroups: every dz fragment feeds two MFMAs
    const bool pair = !(c.p->flags & FD_PLAN_NO_BWD_PAIRING) && !(c.p->tune & FD_TUNE_NO_PW_PAIRING);
    int tn = (K >= 128 && (long)ceil_div(M, 64) * ceil_div(K, 128) >= 200) ? 2 : 1;
    if (pair && !(c.p->tune & FD_TUNE_PW_PAIR_TN2)) tn = 1;   // paired launch: 64 x 64 backward-data tiles (49 KB of LDS per workgroup instead of 74: the weight-gradient workgroups share it) -- measured 554 vs 583 us per bf16 step
    const int m_tiles = ceil_div(M, 64), k_tiles = ceil_div(K, 64 * tn);
    const size_t lds_d = FD_PW_DGRAD_H16_RING(L.n64, tn) + (size_t)4 * 64 * tn * 4;     // ring of min(3, N tiles) stages (>= the epilogue's fp32 tiles) + statistics
    const bool add = P.skip_consumer >= 0;
    const unsigned n_dgrad = (unsigned)((m_tiles + 7) / 8 * 8 * k_tiles);
    if (pair) {
        const size_t lds = std::max(lds_d, FD_PW_WGRAD_H16_LDS(1));
        const int tiles_w = n_tiles * k_tiles_w;
#define FD_PWBWD_H16(ADDV, TNV)                                                                                                                    \
    do {                                                                                                                                           \
        (void)hipFuncSetAttribute((const void *)fd_pw_bwd_h16<T, ACT_IN, ADDV, TNV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);        \
        FD_LAUNCH((fd_pw_bwd_h16<T, ACT_IN, ADDV, TNV>), dim3(n_dgrad + (unsigned)(tiles_w * splits)), dim3(256), lds, c.s, G, twt<T>(c.p, L.wtt_off), twt<T>(c.p, P.z_off), \
                  tws(c.p, P.st_off), ADDV ? twt<T>(c.p, P.sg_off) : (const T *)nullptr, twt<T>(c.p, P.g_off), bwd_rows(c.p, L.d.src), tws(c.p, L.wp_off), M, N, K, L.n64, \
                  m_tiles, k_tiles, (int)n_dgrad, k_tiles_w, tiles_w, rows, (FD_PW_BWD_W_FIRST && (unsigned)(tiles_w * splits) < n_dgrad) ? tiles_w * splits : 0); \
    } while (0)
        if (add) { if (tn == 2) FD_PWBWD_H16(1, 2); else FD_PWBWD_H16(1, 1); }
        else { if (tn == 2) FD_PWBWD_H16(0, 2); else FD_PWBWD_H16(0, 1); }
#undef FD_PWBWD_H16
        if ((rc = check_launch("fd_pw_bwd_h16"))) return rc;
        return defer_weights(c, tws(c.p, L.wp_off), splits, N * K, 0, 0, c.grads[i].conv_weight);
    }
    {
        // (two k tiles per workgroup -- fd_pw_wgrad_h16<.., 2>, the staged dz tile feeding twice the MFMAs -- measured slower: 22.3 vs 20.9 us on the
        // 512 x 512 units, 3 instead of 5 workgroups per CU and half as many of them)
        FD_LAUNCH((fd_pw_wgrad_h16<T, ACT_IN, 1>), dim3(n_tiles * k_tiles_w, splits), dim3(256), FD_PW_WGRAD_H16_LDS(1), c.s, G, twt<T>(c.p, P.z_off), tws(c.p, P.st_off),
                  tws(c.p, L.wp_off), M, N, K, k_tiles_w, rows);
        if ((rc = check_launch("fd_pw_wgrad_h16"))) return rc;
        if ((rc = defer_weights(c, tws(c.p, L.wp_off), splits, N * K, 0, 0, c.grads[i].conv_weight))) return rc;
    }
    {
        dim3 grid(n_dgrad);
#define FD_DGRAD_H16(ADDV, TNV)                                                                                                                    \
    do {                                                                                                                                           \
        (void)hipFuncSetAttribute((const void *)fd_pw_dgrad_h16<T, ACT_IN, ADDV, TNV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_d);    \
        FD_LAUNCH((fd_pw_dgrad_h16<T, ACT_IN, ADDV, TNV>), grid, dim3(256), lds_d, c.s, G, twt<T>(c.p, L.wtt_off), twt<T>(c.p, P.z_off), tws(c.p, P.st_off), \
                  ADDV ? twt<T>(c.p, P.sg_off) : (const T *)nullptr, twt<T>(c.p, P.g_off), bwd_rows(c.p, L.d.src), M, N, K, L.n64, m_tiles, k_tiles);          \
    } while (0)
        if (add) { if (tn == 2) FD_DGRAD_H16(1, 2); else FD_DGRAD_H16(1, 1); }
        else { if (tn == 2) FD_DGRAD_H16(0, 2); else FD_DGRAD_H16(0, 1); }
#undef FD_DGRAD_H16
        return check_launch("fd_pw_dgrad_h16");
    }
}

template <int ACT_IN>
int launch_pw_bwd(BwdCtx &c, int i)
{
    TLayer &L = c.p->layers[i];
    TLayer &P = c.p->layers[L.d.src];
    const int M = (int)L.M, N = L.d.cout, K = L.d.cin;
    const float *G = tws(c.p, L.g_off), *Z = tws(c.p, L.z_off), *coef = tws(c.p, L.coef_off);
    // weights: dW[N][K], reduction over M split across workgroups;  data: G_src[M][K], 64 x 64 tiles (both kernels tile K by 64)
    const int n_tiles = ceil_div(N, 64), k_tiles = ceil_div(K, 64), m_tiles = ceil_div(M, 64);
    int splits = std::max(1, std::min(ceil_div(FD_WGRAD_TARGET_WGS_F32, (long)n_tiles * k_tiles), ceil_div(M, 256)));
    const int rows = ceil_div(ceil_div(M, splits), 64) * 64;
    splits = ceil_div(M, rows);
    if ((size_t)splits * N * K > L.wp_elems) return fail(FD_ERR_STATE, "weight-gradient partial region too small");
    const size_t lds_w = (size_t)FD_BWD_STAGES * 3 * 32 * 64 * 4;
    const int N32 = (N + 31) / 32 * 32;
    const size_t lds_d = ((size_t)FD_BWD_STAGES * (2 * 64 * 32 + 32 * 64) + 4 * N32 + 256) * 4;
    const bool add = P.skip_consumer >= 0;
    const unsigned n_dgrad = (unsigned)((m_tiles + 7) / 8 * 8 * k_tiles);
    int rc;
    if (!(c.p->flags & FD_PLAN_NO_BWD_PAIRING) && !(c.p->tune & FD_TUNE_NO_PW_PAIRING)) {
        const size_t lds = std::max(lds_w, lds_d);
        const int tiles_w = n_tiles * k_tiles;
        const dim3 grid(n_dgrad + (unsigned)(tiles_w * splits));
        const int n_w = (FD_PW_BWD_W_FIRST_F32 && (unsigned)(tiles_w * splits) < n_dgrad) ? tiles_w * splits : 0;
        if (add) {
            (void)hipFuncSetAttribute((const void *)fd_pw_bwd_f32<ACT_IN, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            FD_LAUNCH((fd_pw_bwd_f32<ACT_IN, 1>), grid, dim3(256), lds, c.s, G, Z, coef, c.params[i].conv_weight, tws(c.p, P.z_off), tws(c.p, P.st_off),
                      tws(c.p, P.sg_off), tws(c.p, P.g_off), bwd_rows(c.p, L.d.src), tws(c.p, L.wp_off), M, N, K, m_tiles, k_tiles, (int)n_dgrad, tiles_w, rows, n_w);
        } else {
            (void)hipFuncSetAttribute((const void *)fd_pw_bwd_f32<ACT_IN, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            FD_LAUNCH((fd_pw_bwd_f32<ACT_IN, 0>), grid, dim3(256), lds, c.s, G, Z, coef, c.params[i].conv_weight, tws(c.p, P.z_off), tws(c.p, P.st_off),
                      (const float *)nullptr, tws(c.p, P.g_off), bwd_rows(c.p, L.d.src), tws(c.p, L.wp_off), M, N, K, m_tiles, k_tiles, (int)n_dgrad, tiles_w, rows, n_w);
        }
        if ((rc = check_launch("fd_pw_bwd_f32"))) return rc;
        return defer_weights(c, tws(c.p, L.wp_off), splits, N * K, 0, 0, c.grads[i].conv_weight);
    }
    {
        (void)hipFuncSetAttribute((const void *)fd_pw_wgrad_f32<ACT_IN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_w);
            FD_LAUNCH((fd_pw_wgrad_f32<ACT_IN>), dim3(n_tiles * k_tiles, splits), dim3(256), lds_w, c.s, G, Z, coef, tws(c.p, P.z_off), tws(c.p, P.st_off),
                  tws(c.p, L.wp_off), M, N, K, k_tiles, rows);
        if ((rc = check_launch("fd_pw_wgrad_f32"))) return rc;
        if ((rc = defer_weights(c, tws(c.p, L.wp_off), splits, N * K, 0, 0, c.grads[i].conv_weight))) return rc;
    }
    {
        dim3 grid(n_dgrad);
        if (add) {
            (void)hipFuncSetAttribute((const void *)fd_pw_dgrad_f32<ACT_IN, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_d);
            FD_LAUNCH((fd_pw_dgrad_f32<ACT_IN, 1>), grid, dim3(256), lds_d, c.s, G, Z, coef, c.params[i].conv_weight, tws(c.p, P.z_off), tws(c.p, P.st_off),
                      tws(c.p, P.sg_off), tws(c.p, P.g_off), bwd_rows(c.p, L.d.src), M, N, K, m_tiles, k_tiles);
        } else {
            (void)hipFuncSetAttribute((const void *)fd_pw_dgrad_f32<ACT_IN, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_d);
            FD_LAUNCH((fd_pw_dgrad_f32<ACT_IN, 0>), grid, dim3(256), lds_d, c.s, G, Z, coef, c.params[i].conv_weight, tws(c.p, P.z_off), tws(c.p, P.st_off),
                      (const float *)nullptr, tws(c.p, P.g_off), bwd_rows(c.p, L.d.src), M, N, K, m_tiles, k_tiles);
        }
        return check_launch("fd_pw_dgrad_f32");
    }
}

template <typename T>
int train_backward_t(fd_train_plan *plan, const fd_layer_params *params, const fd_layer_grads *grads, int32_t n_layers,
                     const void *dy, int32_t from_layer, int32_t to_layer, void *stream)
{
    constexpr bool F32 = std::is_same<T, float>::value;
    BwdCtx c{plan, params, grads, static_cast<hipStream_t>(stream)};
    hipStream_t s = c.s;
    int rc;
    // ---- head
    const int hi = n_layers - 1;
    TLayer &Hd = plan->layers[hi];
    TLayer &Hp = plan->layers[Hd.d.src];
    if (from_layer == hi) {
        fd_hs().trace_layer = hi;
        if (!plan->bwd_stats_clean) {       // a second backward after one forward: the backward rows hold the previous pass's sums
            for (int i = 0; i < n_layers; ++i)
                if (hipMemsetAsync(plan->ws + plan->layers[i].sb_off, 0, stat_rows_bytes(plan->layers[i].nr_cap, plan->layers[i].d.cout), s) != hipSuccess) return fail(FD_ERR_HIP, "hipMemsetAsync(statistics rows) failed");
        }
        plan->bwd_stats_clean = false;
        const int nb = std::min(ceil_div(Hd.M, 256), 512);     // (grid-stride: one addition to the head's single statistics channel per workgroup)
        if (Hd.d.act == FD_ACT_RELU6) FD_LAUNCH((fd_head_bwd_reduce_f32<FD_ACT_RELU6_>), dim3(nb), dim3(256), 0, s, static_cast<const float *>(dy), tws(plan, Hd.z_off), tws(plan, Hd.st_off), tws(plan, Hd.g_off), bwd_rows(plan, hi), Hd.M, Hd.out_h, Hd.out_w, Hd.d.upsample);
        else FD_LAUNCH((fd_head_bwd_reduce_f32<FD_ACT_RELU_>), dim3(nb), dim3(256), 0, s, static_cast<const float *>(dy), tws(plan, Hd.z_off), tws(plan, Hd.st_off), tws(plan, Hd.g_off), bwd_rows(plan, hi), Hd.M, Hd.out_h, Hd.out_w, Hd.d.upsample);
        if ((rc = check_launch("fd_head_bwd_reduce_f32"))) return rc;
        if ((rc = bn_bwd_finalize(c, hi))) return rc;
        constexpr int PPB = 16;
        const int nb2 = ceil_div(Hd.M, 32 * PPB);
        const size_t lds = (size_t)32 * Hd.d.cin * 3 * 4;
        float *wpart = tws(plan, Hd.wp_off);
        if ((size_t)nb2 * Hd.d.cin > Hd.wp_elems) return fail(FD_ERR_STATE, "weight-gradient partial region too small for the head");
        if (Hp.d.act == FD_ACT_RELU6) FD_LAUNCH((fd_head_bwd<T, FD_ACT_RELU6_, PPB>), dim3(nb2), dim3(256), lds, s, tws(plan, Hd.g_off), tws(plan, Hd.z_off), tws(plan, Hd.coef_off), twt<T>(plan, Hp.z_off), tws(plan, Hp.st_off), params[hi].conv_weight, twt<T>(plan, Hp.g_off), bwd_rows(plan, Hd.d.src), wpart, Hd.M, Hd.d.cin);
        else FD_LAUNCH((fd_head_bwd<T, FD_ACT_RELU_, PPB>), dim3(nb2), dim3(256), lds, s, tws(plan, Hd.g_off), tws(plan, Hd.z_off), tws(plan, Hd.coef_off), twt<T>(plan, Hp.z_off), tws(plan, Hp.st_off), params[hi].conv_weight, twt<T>(plan, Hp.g_off), bwd_rows(plan, Hd.d.src), wpart, Hd.M, Hd.d.cin);
        if ((rc = check_launch("fd_head_bwd"))) return rc;
        if ((rc = defer_weights(c, wpart, nb2, Hd.d.cin, 0, 0, grads[hi].conv_weight))) return rc;
        // the BatchNorm partial sums of the head's producer are in its statistics rows
        if ((rc = finalize_or_defer(c, Hd.d.src))) return rc;
    }
    // ---- remaining units in reverse order; invariant: coef_i and the BN grads of unit i are final when unit i is processed
    for (int i = std::min(hi - 1, (int)from_layer); i >= to_layer; --i) {
        TLayer &L = plan->layers[i];
        const fd_layer_desc &d = L.d;
        fd_hs().trace_layer = i;
        switch (d.op) {
        case FD_OP_STEM: {
            const int nblocks_w = ceil_div((long)plan->B * L.out_h * L.out_w, 256);   // blocks of 256 pixels of the flat [B*Ho*Wo] order (they may straddle images)
            const int nb_w = std::min(nblocks_w, 512);       // workgroups walk them grid-stride
            if (d.cout > 64) return fail(FD_ERR_INVALID, "stem weight gradient supports at most 64 output channels");
            float *wpart = tws(plan, L.wp_off);
            if constexpr (!F32) {
                // 16-bit plans, the 32-channel stem: row-walking fp32 kernel (fd_kernels_dw5p_bwd.h: fd_stem_wgrad_rows), one partial row per workgroup
                if (L.stemw_groups) {
                    const int wgs = ceil_div((long)L.stemw_groups * ceil_div(L.out_h, L.stemw_bh), 4), rows_w = wgs * plan->B;
#define FD_STEMW(CL_)                                                                                                                                     \
    FD_LAUNCH((fd_stem_wgrad_rows<T, CL_, FD_STEMW_CPL>), dim3((unsigned)wgs, (unsigned)plan->B), dim3(256), 0, s, static_cast<const float *>(plan->x_saved), twt<T>(plan, L.g_off), \
              twt<T>(plan, L.z_off), tws(plan, L.coef_off), wpart, L.in_h, L.in_w, L.stemw_groups, L.stemw_bh)
                    if (d.cout == 32) FD_STEMW(32 / FD_STEMW_CPL); else if (d.cout == 16) FD_STEMW(16 / FD_STEMW_CPL); else FD_STEMW(8 / FD_STEMW_CPL);
#undef FD_STEMW
                    if ((rc = check_launch("fd_stem_wgrad_rows"))) return rc;
                    if ((rc = defer_weights(c, wpart, rows_w, 27 * d.cout, 0, 0, grads[i].conv_weight))) return rc;
                    break;
                }
            }
            FD_LAUNCH((fd_stem_wgrad<T>), dim3(nb_w), dim3(256), (size_t)(256 * 33 + 256 * (d.cout + 1)) * 4, s, static_cast<const float *>(plan->x_saved), twt<T>(plan, L.g_off), twt<T>(plan, L.z_off), tws(plan, L.coef_off), wpart, plan->B, L.in_h, L.in_w, d.cout, nblocks_w);
            if ((rc = check_launch("fd_stem_wgrad"))) return rc;
            if ((rc = defer_weights(c, wpart, nb_w, 27 * d.cout, 0, 0, grads[i].conv_weight))) return rc;
            break;
        }
        case FD_OP_DW:
            if ((rc = launch_dw_bwd<T>(c, i)) || (rc = finalize_or_defer(c, d.src))) return rc;
            break;
        case FD_OP_PW: {
            const TLayer &P = plan->layers[d.src];
            if constexpr (F32) rc = P.d.act == FD_ACT_RELU6 ? launch_pw_bwd<FD_ACT_RELU6_>(c, i) : launch_pw_bwd<FD_ACT_RELU_>(c, i);
            else rc = P.d.act == FD_ACT_RELU6 ? launch_pw_bwd_h16<T, FD_ACT_RELU6_>(c, i) : launch_pw_bwd_h16<T, FD_ACT_RELU_>(c, i);
            if (rc) return rc;
            if ((rc = finalize_or_defer(c, d.src))) return rc;
            break;
        }
        }
    }
    fd_hs().trace_layer = -1;
    return flush_weights(c);                                  // one launch reduces the weight-gradient partials of every unit of this range
}

}  // namespace

extern "C" {

int fd_train_backward(fd_train_plan *plan, const fd_layer_params *params, const fd_layer_grads *grads, int32_t n_layers,
                      const void *dy, void *stream)
{
    return fd_train_backward_range(plan, params, grads, n_layers, dy, n_layers - 1, 0, stream);
}

int fd_train_backward_range(fd_train_plan *plan, const fd_layer_params *params, const fd_layer_grads *grads, int32_t n_layers,
                            const void *dy, int32_t from_layer, int32_t to_layer, void *stream)
{
    if (!plan || !params || !grads || !dy) return fail(FD_ERR_INVALID, "null argument");
    if (!plan->ws || !plan->forward_done) return fail(FD_ERR_STATE, "fd_train_backward needs a preceding fd_train_forward on this plan");
    if (n_layers != (int)plan->layers.size()) return fail(FD_ERR_INVALID, "expected %zu layers", plan->layers.size());
    if (from_layer < to_layer || from_layer >= n_layers || to_layer < 0) return fail(FD_ERR_INVALID, "bad layer range %d..%d", from_layer, to_layer);
    for (int i = 0; i < n_layers; ++i)
        if (!grads[i].conv_weight || !grads[i].bn_weight || !grads[i].bn_bias) return fail(FD_ERR_INVALID, "layer %d: null gradient pointer", i);
    // the backward kernels read the live conv weights with 16-byte loads; dy and every gradient tensor are accessed element by element
    for (int i = 0; i < n_layers; ++i)
        if (misaligned(params[i].conv_weight, 16)) return fail(FD_ERR_INVALID, "layer %d: conv_weight must be 16-byte aligned", i);
    return plan->dtype == FD_BF16 ? train_backward_t<fd_bf16>(plan, params, grads, n_layers, dy, from_layer, to_layer, stream)
                                  : train_backward_t<float>(plan, params, grads, n_layers, dy, from_layer, to_layer, stream);
}

int fd_cast_gradients(const void *src, void *dst, int64_t numel, int32_t to_bf16, void *stream);

/* ---- data-parallel gradient exchange issued by the library itself: RCCL all-reduce over xGMI (the reference's only multi-GPU
 * idiom is torch.nn.DataParallel, imagenet/mobilenet.py:68).  RCCL is bound at RUN time (dlopen "librccl.so.1": inside a torch process that is the
 * RCCL torch itself loaded, by SONAME; a torch-free host gets the system library), so the library has no link-time dependency on it and loads on
 * hosts without RCCL.  One communicator + one non-blocking HIP stream + one event per bucket; no host synchronisation anywhere.
 * The binding is injectable (fd_comm_bind_library, csrc/fd_tuning.h): the CPU test tier binds tests/rccl_stub -- the four nccl* entry points over POSIX
 * shared memory -- to the EMULATOR build, so that this very code (bucket tiling, the 16-bit cast -> sum -> cast back, the order of the hand-overs, the
 * mean folded into fd_sgd_step) runs at world size 2 without a GPU.  Without a bound library the emulator build offers a one-rank communicator whose
 * all-reduce is the identity. ---- */
#include <dlfcn.h>
#ifdef FD_EMU
#define hipEventReleaseToDevice 0
inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }
#endif
struct fd_comm {
    void *comm = nullptr;                 // ncclComm_t (null: the emulator's one-rank communicator, all-reduce = identity)
    hipStream_t stream = nullptr;         // the collectives' stream
    std::vector<hipEvent_t> bucket_done;  // recorded on the compute stream after a bucket's last backward kernel
    hipEvent_t all_done = nullptr, t0 = nullptr, t1 = nullptr, tb = nullptr;   // t0 / t1: first collective issued / last one finished; tb: backward finished on the compute stream (timing enabled)
    int rank = 0, world = 1;
    bool timed = false;                   // t0 / t1 hold a pair of the last fd_train_backward_allreduce
    bool elide = false;                   // measurement hook (fd_tuning.h: fd_comm_elide_collectives): everything but the ncclAllReduce calls themselves
};

extern "C++" {
namespace {
struct fd_nccl_uid { char internal[FD_COMM_ID_BYTES]; };
struct RcclApi {
    int (*GetUniqueId)(fd_nccl_uid *) = nullptr;
    int (*CommInitRank)(void **, int, fd_nccl_uid, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
};
std::string &rccl_path() { static std::string p; return p; }      // set by fd_comm_bind_library before the first use
RcclApi &rccl()
{
    static RcclApi api = [] {
        RcclApi a;
        void *h = nullptr;
        if (!rccl_path().empty()) h = dlopen(rccl_path().c_str(), RTLD_NOW | RTLD_LOCAL);
#ifndef FD_EMU
        else for (const char *name : {"librccl.so.1", "librccl.so"}) if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
#endif
        if (!h) return a;
        a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
        a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
        a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(h, "ncclAllReduce"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
        a.ok = a.GetUniqueId && a.CommInitRank && a.AllReduce && a.CommDestroy;
        return a;
    }();
    return api;
}
int rccl_fail(const char *what, int rc)
{
    const RcclApi &a = rccl();
    return fail(FD_ERR_HIP, "%s: RCCL error %d (%s)", what, rc, a.GetErrorString ? a.GetErrorString(rc) : "?");
}
constexpr int kNcclSum = 0, kNcclFloat32 = 7, kNcclBfloat16 = 9;    // rccl.h: ncclRedOp_t / ncclDataType_t
#ifdef FD_EMU
constexpr bool kOneRankWithoutLibrary = true;     // the emulator's fallback communicator
#else
constexpr bool kOneRankWithoutLibrary = false;
#endif
}  // namespace
}  // extern "C++"

int fd_comm_bind_library(const char *path)
{
    if (!path || !*path) return fail(FD_ERR_INVALID, "fd_comm_bind_library: empty path");
    if (!rccl_path().empty() && rccl_path() != path) return fail(FD_ERR_STATE, "fd_comm_bind_library: already bound to %s", rccl_path().c_str());
    if (rccl_path().empty()) {
        // the candidate is opened and checked BEFORE the path is committed: a library that cannot be loaded (or lacks an entry point) must not leave the
        // process bound to it for good -- the one-time binding below would then never try librccl.so.1 or another path again
        void *h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        if (!h) return fail(FD_ERR_STATE, "fd_comm_bind_library: %s cannot be loaded (%s)", path, dlerror());
        for (const char *sym : {"ncclGetUniqueId", "ncclCommInitRank", "ncclAllReduce", "ncclCommDestroy"})
            if (!dlsym(h, sym)) { dlclose(h); return fail(FD_ERR_STATE, "fd_comm_bind_library: %s does not provide %s", path, sym); }
    }
    rccl_path() = path;
    if (!rccl().ok) return fail(FD_ERR_STATE, "fd_comm_bind_library: %s does not provide ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy (or the binding was made before this call)", path);
    return FD_OK;
}

int fd_comm_unique_id(void *id_out)
{
    if (!id_out) return fail(FD_ERR_INVALID, "null argument");
    if (!rccl().ok) {
        if (kOneRankWithoutLibrary) { memset(id_out, 0, FD_COMM_ID_BYTES); return FD_OK; }       // (the emulator's one-rank communicator: no rendezvous)
        return fail(FD_ERR_STATE, "librccl.so.1 could not be loaded (or lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy)");
    }
    fd_nccl_uid id{};
    const int rc = rccl().GetUniqueId(&id);
    if (rc) return rccl_fail("ncclGetUniqueId", rc);
    memcpy(id_out, id.internal, FD_COMM_ID_BYTES);
    return FD_OK;
}

int fd_comm_create(const void *id, int32_t rank, int32_t world, fd_comm **out)
{
    if (!id || !out || world <= 0 || rank < 0 || rank >= world) return fail(FD_ERR_INVALID, "fd_comm_create: bad argument (rank %d of %d)", rank, world);
    if (!rccl().ok && !(kOneRankWithoutLibrary && world == 1))
        return fail(FD_ERR_STATE, kOneRankWithoutLibrary ? "the CPU emulator offers a one-rank communicator only unless a collective library is bound (fd_comm_bind_library)" : "librccl.so.1 could not be loaded");
    fd_comm *c = new fd_comm();
    c->rank = rank; c->world = world;
    if (rccl().ok) {
        fd_nccl_uid uid{};
        memcpy(uid.internal, id, FD_COMM_ID_BYTES);
        const int rc = rccl().CommInitRank(&c->comm, world, uid, rank);          // (on the calling thread's current device, like every entry point here)
        if (rc) { delete c; return rccl_fail("ncclCommInitRank", rc); }
    }
    // Every event here is consumed by another stream of the SAME device (or only read for its timestamp): a device-scope release.  A default HIP event
    // performs a SYSTEM-scope fence when it is recorded -- an L2 write-back + invalidate in the middle of backward; measured on one rank: the exchange
    // machinery cost +155 us per step with default events (6 records per step), with or without the ncclAllReduce calls themselves.
    // (a default-priority stream: with the highest priority the one-rank step measured 8.6 ms instead of 2.56 -- the hand-over barriers pre-empt the
    // compute queue)
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->all_done, hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&c->t0, hipEventReleaseToDevice) != hipSuccess || hipEventCreateWithFlags(&c->t1, hipEventReleaseToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&c->tb, hipEventReleaseToDevice) != hipSuccess) {
        fd_comm_destroy(c);
        return fail(FD_ERR_HIP, "fd_comm_create: stream / event creation failed");
    }
    *out = c;
    return FD_OK;
}

void fd_comm_destroy(fd_comm *c)
{
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm && rccl().ok) (void)rccl().CommDestroy(c->comm);
    for (hipEvent_t e : c->bucket_done) (void)hipEventDestroy(e);
    for (hipEvent_t e : {c->all_done, c->t0, c->t1, c->tb}) if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int fd_train_backward_allreduce(fd_train_plan *plan, const fd_layer_params *params, const fd_layer_grads *grads, int32_t n_layers, const void *dy,
                                fd_comm *comm, const fd_grad_bucket *buckets, int32_t n_buckets, void *stream)
{
    if (!comm || !buckets || n_buckets <= 0) return fail(FD_ERR_INVALID, "fd_train_backward_allreduce: null communicator / empty bucket list");
    // the buckets must tile the layers n-1 .. 0 in backward order
    int expect = n_layers - 1;
    for (int b = 0; b < n_buckets; ++b) {
        if (buckets[b].from_layer != expect || buckets[b].to_layer > buckets[b].from_layer || buckets[b].to_layer < 0 || !buckets[b].grad || buckets[b].numel <= 0)
            return fail(FD_ERR_INVALID, "bucket %d: layers %d..%d do not continue the backward order at %d (or null / empty gradient slice)", b, buckets[b].from_layer, buckets[b].to_layer, expect);
        expect = buckets[b].to_layer - 1;
    }
    if (expect != -1) return fail(FD_ERR_INVALID, "the buckets stop at layer %d: they must cover every layer", expect + 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    while ((int)comm->bucket_done.size() < n_buckets) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) return fail(FD_ERR_HIP, "hipEventCreate failed");
        comm->bucket_done.push_back(e);
    }
    comm->timed = false;
    // the summing all-reduce of `count` values in place on the communicator's stream (no library bound, emulator: one rank, the identity)
    auto all_reduce = [&](void *buf, size_t count, bool bf16) -> int {
        if (comm->elide || !comm->comm) return FD_OK;
        const int nrc = rccl().AllReduce(buf, buf, count, bf16 ? kNcclBfloat16 : kNcclFloat32, kNcclSum, comm->comm, comm->stream);
        return nrc ? rccl_fail("ncclAllReduce", nrc) : FD_OK;
    };
    // Whatever happens after the first hand-over, the caller's stream must not run ahead of collectives that are already enqueued on the gradient
    // buffers: every exit below that point -- error or not -- joins the communication stream back into `s`.
    bool handed_over = false;
    auto join = [&]() -> bool {
        return hipEventRecord(comm->all_done, comm->stream) == hipSuccess && hipStreamWaitEvent(s, comm->all_done, 0) == hipSuccess;
    };
    auto bail = [&](int rc) -> int {
        if (handed_over && !join()) (void)hipStreamSynchronize(comm->stream);      // (last resort: the host waits)
        return rc;
    };
    for (int b = 0; b < n_buckets; ++b) {
        const fd_grad_bucket &k = buckets[b];
        int rc = fd_train_backward_range(plan, params, grads, n_layers, dy, k.from_layer, k.to_layer, stream);
        if (rc) return bail(rc);
        // the bucket's gradients are complete on the compute stream: the collective's stream waits for exactly that point
        if (hipEventRecord(comm->bucket_done[b], s) != hipSuccess || hipStreamWaitEvent(comm->stream, comm->bucket_done[b], 0) != hipSuccess)
            return bail(fail(FD_ERR_HIP, "event hand-over to the communication stream failed"));
        handed_over = true;
        if (b == 0) (void)hipEventRecord(comm->t0, comm->stream);
        if (k.grad16) {                                          // 16-bit exchange: convert, all-reduce the bf16 copy, convert back -- all in stream order
            if ((rc = fd_cast_gradients(k.grad, k.grad16, k.numel, 1, comm->stream))) return bail(rc);
            if ((rc = all_reduce(k.grad16, (size_t)k.numel, true))) return bail(rc);
            if ((rc = fd_cast_gradients(k.grad16, k.grad, k.numel, 0, comm->stream))) return bail(rc);
        } else if ((rc = all_reduce(k.grad, (size_t)k.numel, false))) return bail(rc);
    }
    (void)hipEventRecord(comm->tb, s);
    (void)hipEventRecord(comm->t1, comm->stream);
    // whatever the caller enqueues next on its stream (fd_sgd_step) runs after the last collective
    if (!join()) { (void)hipStreamSynchronize(comm->stream); return fail(FD_ERR_HIP, "event hand-over from the communication stream failed"); }
    comm->timed = true;
    return FD_OK;
}

void fd_comm_elide_collectives(fd_comm *comm, int32_t on) { if (comm) comm->elide = on != 0; }

int fd_comm_last_exchange_ms(fd_comm *comm, float *ms_exchange, float *ms_exposed)
{
    if (!comm || !ms_exchange || !ms_exposed) return fail(FD_ERR_INVALID, "null argument");
    if (!comm->timed) return fail(FD_ERR_STATE, "no exchange has been issued on this communicator");
    if (hipEventSynchronize(comm->t1) != hipSuccess || hipEventSynchronize(comm->tb) != hipSuccess || hipEventElapsedTime(ms_exchange, comm->t0, comm->t1) != hipSuccess)
        return fail(FD_ERR_HIP, "event timing failed");
    // exposed: how long after the last backward kernel the last collective ended (an event pair in the "wrong" order is a fully hidden exchange)
    if (hipEventElapsedTime(ms_exposed, comm->tb, comm->t1) != hipSuccess || *ms_exposed < 0.0f) *ms_exposed = 0.0f;
    return FD_OK;
}

int fd_val_transform(const void *rgb_u8, const float *depth, int32_t n, int32_t height, int32_t width, int32_t out_h, int32_t out_w,
                     const int32_t *ymap_device, const int32_t *xmap_device, float *x_out, float *depth_out, void *stream)
{
    if (!rgb_u8 || !ymap_device || !xmap_device || !x_out || n <= 0 || height <= 0 || width <= 0 || out_h <= 0 || out_w <= 0)
        return fail(FD_ERR_INVALID, "fd_val_transform: null/empty argument");
    if ((depth == nullptr) != (depth_out == nullptr)) return fail(FD_ERR_INVALID, "fd_val_transform: depth and depth_out go together");
    const long total = (long)n * out_h * out_w;
    FD_LAUNCH(fd_val_transform_u8, dim3((unsigned)std::min<long>(4096, ceil_div(total, 256))), dim3(256), 0, static_cast<hipStream_t>(stream),
              static_cast<const unsigned char *>(rgb_u8), depth, ymap_device, xmap_device, x_out, depth_out, n, height, width, out_h, out_w);
    return check_launch("fd_val_transform_u8");
}

// scratch of fd_train_transform: [n] frame headers | y1[FD_AUG_MAX_H1] | x1[FD_AUG_MAX_W1] | ytab[n][out_h] | xtab[n][out_w] | stash[n][out_h * out_w] (uint32)
namespace {
struct AugScratch { size_t frames, y1, x1, ytab, xtab, stash, total; };
AugScratch aug_scratch(int32_t n, int32_t oh, int32_t ow)
{
    AugScratch a;
    a.frames = 0;
    a.y1 = align_up((size_t)n * sizeof(fd_aug_frame), 256);
    a.x1 = a.y1 + (size_t)FD_AUG_MAX_H1 * sizeof(int);
    a.ytab = a.x1 + (size_t)FD_AUG_MAX_W1 * sizeof(int);
    a.xtab = align_up(a.ytab + (size_t)n * oh * sizeof(int), 256);
    a.stash = align_up(a.xtab + (size_t)n * ow * sizeof(int), 256);
    a.total = a.stash + (size_t)n * oh * ow * sizeof(unsigned);
    return a;
}
// Can the host read the records where they are?  (Page-locked host memory the device reads in place; everything is host memory in the emulator.)
// -1: the device cannot read the pointer at all (pageable host memory).
int aug_params_host_readable(const void *p)
{
#ifdef FD_EMU
    (void)p;
    return 1;
#else
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    if (a.type == hipMemoryTypeHost) return 1;
    return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) ? 0 : -1;
#endif
}
}  // namespace

size_t fd_train_transform_scratch_bytes(int32_t n, int32_t out_h, int32_t out_w)
{
    if (n <= 0 || out_h <= 0 || out_w <= 0) return 0;
    return aug_scratch(n, out_h, out_w).total;
}

int fd_train_transform(const void *rgb_u8, const float *depth, int32_t n, int32_t height, int32_t width, int32_t out_h, int32_t out_w,
                       const fd_aug_params *params_device, float *x_out, float *depth_out, void *scratch, void *stream)
{
    if (!rgb_u8 || !params_device || !x_out || !scratch || n <= 0 || height <= 0 || width <= 0 || out_h <= 0 || out_w <= 0)
        return fail(FD_ERR_INVALID, "fd_train_transform: null/empty argument");
    if ((depth == nullptr) != (depth_out == nullptr)) return fail(FD_ERR_INVALID, "fd_train_transform: depth and depth_out go together");
    if ((long)out_h * out_w > (1L << 28) || (long)height * width > (1L << 28)) return fail(FD_ERR_INVALID, "fd_train_transform: frame of more than 2^28 pixels");
    if (reinterpret_cast<uintptr_t>(scratch) & 127) return fail(FD_ERR_INVALID, "fd_train_transform: scratch must be 128-byte aligned");
    // Resize(250.0 / iheight) with a float: size = (array(im.size) * f).astype(int)   (reference nyu.py:34, scipy.misc.imresize)
    const double f = 250.0 / height;
    const int h1 = (int)(height * f), w1 = (int)(width * f);
    // Too small: no scale that fd_aug_record_check admits (s <= FD_AUG_MAX_SCALE) makes the resized image cover the crop.
    if ((int)(h1 * FD_AUG_MAX_SCALE) < FD_AUG_CROP_H || (int)(w1 * FD_AUG_MAX_SCALE) < FD_AUG_CROP_W)
        return fail(FD_ERR_INVALID, "fd_train_transform: a %d x %d frame is too small for the %d x %d crop (it resizes to %d x %d, and to %g times that at most)",
                    height, width, FD_AUG_CROP_H, FD_AUG_CROP_W, h1, w1, (double)FD_AUG_MAX_SCALE);
    // h1 <= 250 by construction; the first resize's column table in scratch holds FD_AUG_MAX_W1 entries.
    if (h1 > FD_AUG_MAX_H1 || w1 > FD_AUG_MAX_W1)
        return fail(FD_ERR_INVALID, "fd_train_transform: a %d x %d frame resizes to %d x %d, beyond the %d x %d the tables are planned for", height, width, h1, w1,
                    FD_AUG_MAX_H1, FD_AUG_MAX_W1);
    // The records live where the device reads them.  Where the host can read them too they are checked here; in plain device memory the table step
    // applies the same rule (fd_aug_record_check) and a refused frame comes out as zeros -- no read-back, nothing here synchronises.
    const int readable = aug_params_host_readable(params_device);
    if (readable < 0) return fail(FD_ERR_INVALID, "fd_train_transform: params_device is not memory the device can read");
    if (readable > 0)
        for (int i = 0; i < n; ++i) {
            const fd_aug_params &p = params_device[i];
            switch (fd_aug_record_check(p, h1, w1)) {
            case 1: return fail(FD_ERR_INVALID, "fd_train_transform: frame %d: order (%d, %d, %d) is not a permutation of {0, 1, 2}", i, p.order[0], p.order[1], p.order[2]);
            case 2: return fail(FD_ERR_INVALID, "fd_train_transform: frame %d: s = %g is not in (0, %g]", i, p.s, (double)FD_AUG_MAX_SCALE);
            case 3: return fail(FD_ERR_INVALID, "fd_train_transform: frame %d: s = %g resizes %d x %d to %d x %d, smaller than the %d x %d crop", i, p.s, h1, w1,
                                (int)(h1 * p.s), (int)(w1 * p.s), FD_AUG_CROP_H, FD_AUG_CROP_W);
            case 4: return fail(FD_ERR_INVALID, "fd_train_transform: frame %d: a colour factor (%g, %g, %g) or the angle (%g) is not finite", i, (double)p.brightness, (double)p.contrast,
                                (double)p.saturation, p.angle);
            default: break;
            }
        }
    const AugScratch a = aug_scratch(n, out_h, out_w);
    char *base = static_cast<char *>(scratch);
    fd_aug_frame *frames = reinterpret_cast<fd_aug_frame *>(base + a.frames);
    int *y1 = reinterpret_cast<int *>(base + a.y1), *x1 = reinterpret_cast<int *>(base + a.x1);
    int *ytab = reinterpret_cast<int *>(base + a.ytab), *xtab = reinterpret_cast<int *>(base + a.xtab);
    unsigned *stash = reinterpret_cast<unsigned *>(base + a.stash);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long px = (long)out_h * out_w;
    FD_LAUNCH(fd_aug_tables, dim3((unsigned)n + 1), dim3(256), 0, s, params_device, frames, y1, x1, ytab, xtab, n, height, width, h1, w1, out_h, out_w);
    int rc = check_launch("fd_aug_tables");
    if (rc) return rc;
    FD_LAUNCH(fd_aug_gather, dim3((unsigned)ceil_div(px, 256L * FD_AUG_PIX_PER_ITEM), (unsigned)n), dim3(256), 0, s, static_cast<const unsigned char *>(rgb_u8), depth,
              frames, y1, x1, ytab, xtab, stash, depth_out, height, width, h1, w1, out_h, out_w);
    if ((rc = check_launch("fd_aug_gather"))) return rc;
    FD_LAUNCH(fd_aug_apply, dim3((unsigned)ceil_div(px, 1024), (unsigned)n), dim3(256), 0, s, frames, stash, x_out, out_h, out_w);
    return check_launch("fd_aug_apply");
}

// scratch of fd_depth_rows: float [n][FD_VIZ_MAX_PARTS][2], the (min, max) partials of fd_viz_range; every slot that is read has been written by this call
size_t fd_depth_rows_scratch_bytes(int32_t n)
{
    if (n <= 0) return 0;
    return (size_t)n * FD_VIZ_MAX_PARTS * 2 * sizeof(float);
}

int fd_depth_rows(const float *x_nchw, const float *map0, const float *map1, const float *map2, int32_t n, int32_t h, int32_t w, const float *range_device,
                  uint8_t *canvas, int64_t pitch_bytes, void *scratch, void *stream)
{
    if (n <= 0 || h <= 0 || w <= 0) return fail(FD_ERR_INVALID, "fd_depth_rows: n, h and w must be positive (got %d, %d, %d)", n, h, w);
    if (!map0) return fail(FD_ERR_INVALID, "fd_depth_rows: map0 is required");
    if (!map1 && map2) return fail(FD_ERR_INVALID, "fd_depth_rows: map2 given without map1 (the maps are map0, map1, map2 in order)");
    if (!canvas) return fail(FD_ERR_INVALID, "fd_depth_rows: canvas is NULL");
    const int k = 1 + (map1 ? 1 : 0) + (map2 ? 1 : 0), panels = k + (x_nchw ? 1 : 0);
    const int64_t row = (int64_t)panels * w * 3;
    if (pitch_bytes < row)
        return fail(FD_ERR_INVALID, "fd_depth_rows: pitch_bytes = %lld is smaller than a row of %d panels of %d pixels (%lld bytes)", (long long)pitch_bytes, panels, w,
                    (long long)row);
    if (!range_device && !scratch) return fail(FD_ERR_INVALID, "fd_depth_rows: scratch is NULL and no range_device is given (fd_depth_rows_scratch_bytes(n) bytes)");
    if (reinterpret_cast<uintptr_t>(range_device) & 3 || reinterpret_cast<uintptr_t>(scratch) & 3)
        return fail(FD_ERR_INVALID, "fd_depth_rows: range_device and scratch must be 4-byte aligned");
    const long px = (long)h * w;
    auto al = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    int flags = 0;
    if (w % 4 == 0 && pitch_bytes % 4 == 0 && al(canvas, 4)) flags |= FD_VIZ_STORE4;
    if (w % 4 == 0 && al(x_nchw, 16) && al(map0, 16) && al(map1, 16) && al(map2, 16)) flags |= FD_VIZ_LOAD4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *partials = static_cast<float *>(scratch);
    int parts = 0;
    if (!range_device) {
        parts = std::max(1, std::min(FD_VIZ_MAX_PARTS, ceil_div((long)k * px, FD_VIZ_PART_ELEMS)));
        FD_LAUNCH(fd_viz_range, dim3((unsigned)n, (unsigned)parts), dim3(256), 0, s, map0, map1, map2, partials, px, flags & FD_VIZ_LOAD4);
        const int rc = check_launch("fd_viz_range");
        if (rc) return rc;
    }
    // 256 work-items x 4 pixels per workgroup and pass; at most 1024 workgroups per frame, the loop takes the rest
    const long items = (long)h * panels * ((w + 3) / 4);
    const unsigned gy = (unsigned)std::min(1024L, (items + 255) / 256);
    FD_LAUNCH(fd_viz_paint, dim3((unsigned)n, gy), dim3(256), 0, s, x_nchw, map0, map1, map2, range_device, partials, parts, canvas, (long)pitch_bytes, h, w, k, flags);
    return check_launch("fd_viz_paint");
}

int fd_cast_gradients(const void *src, void *dst, int64_t numel, int32_t to_bf16, void *stream)
{
    if (!src || !dst || numel <= 0) return fail(FD_ERR_INVALID, "fd_cast_gradients: null/empty argument");
    // 4 values per work-item: 16-byte accesses on the fp32 side, 8-byte accesses on the bf16 side -- each side is tested against ITS access width
    // (bucket starts are multiples of 4 elements: a bf16 pointer at 8 mod 16 is fine and must not drop the whole bucket to one element per work-item)
    const uintptr_t p32 = reinterpret_cast<uintptr_t>(to_bf16 ? src : dst), p16 = reinterpret_cast<uintptr_t>(to_bf16 ? dst : src);
    const bool al = (p32 & 15) == 0 && (p16 & 7) == 0;
    const long n4 = al ? (long)(numel >> 2) : 0;
    const unsigned nb = (unsigned)std::min<long>(2048, ceil_div((long)std::max<int64_t>(numel / 4, 1), 256));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (to_bf16) FD_LAUNCH(fd_cast_f32_bf16, dim3(nb), dim3(256), 0, s, static_cast<const float *>(src), static_cast<fd_bf16 *>(dst), n4, (long)numel);
    else FD_LAUNCH(fd_cast_bf16_f32, dim3(nb), dim3(256), 0, s, static_cast<const fd_bf16 *>(src), static_cast<float *>(dst), n4, (long)numel);
    return check_launch("fd_cast_gradients");
}

size_t fd_depth_metrics_scratch_bytes(void) { return (size_t)1024 * 10 * sizeof(double); }

int fd_depth_metrics(const void *output, const void *target, int64_t numel, double *sums_device, void *scratch, void *stream)
{
    if (!output || !target || !sums_device || !scratch || numel <= 0) return fail(FD_ERR_INVALID, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = (int)std::min<int64_t>(1024, (numel + 255) / 256);
    FD_LAUNCH(fd_depth_metrics_f32, dim3(nb), dim3(256), 0, s, static_cast<const float *>(output), static_cast<const float *>(target), (long)numel, static_cast<double *>(scratch));
    int rc = check_launch("fd_depth_metrics_f32");
    if (rc) return rc;
    FD_LAUNCH(fd_depth_metrics_final_f32, dim3(1), dim3(64), 0, s, static_cast<const double *>(scratch), nb, sums_device);
    return check_launch("fd_depth_metrics_final_f32");
}

size_t fd_depth_metrics_frames_scratch_bytes(int32_t n_frames) { return (size_t)std::max(n_frames, 1) * 64 * 10 * sizeof(double); }

int fd_depth_metrics_frames(const void *output, const void *target, int32_t n_frames, int64_t frame_numel, double *sums_device, void *scratch, void *stream)
{
    if (!output || !target || !sums_device || !scratch || n_frames <= 0 || frame_numel <= 0) return fail(FD_ERR_INVALID, "null argument / empty batch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = (int)std::min<int64_t>(64, (frame_numel + 255) / 256);
    FD_LAUNCH(fd_depth_metrics_f32, dim3(nb, n_frames), dim3(256), 0, s, static_cast<const float *>(output), static_cast<const float *>(target), (long)frame_numel,
              static_cast<double *>(scratch));
    int rc = check_launch("fd_depth_metrics_f32");
    if (rc) return rc;
    FD_LAUNCH(fd_depth_metrics_final_f32, dim3(n_frames), dim3(64), 0, s, static_cast<const double *>(scratch), nb, sums_device);
    return check_launch("fd_depth_metrics_final_f32");
}

size_t fd_l1_loss_scratch_bytes(int64_t numel) { (void)numel; return 2 * 1024 * sizeof(float); }   // masked form: (sum, count) per workgroup

int fd_l1_loss(const void *pred, const void *target, void *dpred, float *loss_out, int64_t numel, void *scratch, void *stream)
{
    if (!pred || !target || !dpred || !loss_out || !scratch || numel <= 0) return fail(FD_ERR_INVALID, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = (int)std::min<int64_t>(1024, (numel + 255) / 256);
    const float inv = 1.0f / (float)numel;
    FD_LAUNCH(fd_l1_loss_f32, dim3(nb), dim3(256), 0, s, static_cast<const float *>(pred), static_cast<const float *>(target), static_cast<float *>(dpred),
              static_cast<float *>(scratch), (long)numel, inv);
    int rc = check_launch("fd_l1_loss_f32");
    if (rc) return rc;
    FD_LAUNCH(fd_l1_loss_final_f32, dim3(1), dim3(64), 0, s, static_cast<const float *>(scratch), nb, inv, loss_out);
    return check_launch("fd_l1_loss_final_f32");
}

int fd_l1_loss_masked(const void *pred, const void *target, void *dpred, float *loss_out, int64_t numel, void *scratch, void *stream)
{
    if (!pred || !target || !dpred || !loss_out || !scratch || numel <= 0) return fail(FD_ERR_INVALID, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = (int)std::min<int64_t>(1024, (numel + 255) / 256);
    FD_LAUNCH(fd_l1_masked_partial_f32, dim3(nb), dim3(256), 0, s, static_cast<const float *>(pred), static_cast<const float *>(target), static_cast<float *>(scratch), (long)numel);
    int rc = check_launch("fd_l1_masked_partial_f32");
    if (rc) return rc;
    FD_LAUNCH(fd_l1_masked_apply_f32, dim3(nb), dim3(256), 0, s, static_cast<const float *>(pred), static_cast<const float *>(target), static_cast<const float *>(scratch), nb,
              static_cast<float *>(dpred), loss_out, (long)numel);
    return check_launch("fd_l1_masked_apply_f32");
}

int fd_sgd_step(const fd_sgd_tensor *table_device, int32_t n_tensors, int64_t total_numel, float lr, float momentum, float weight_decay,
                float grad_scale, int32_t first_step, void *stream)
{
    if (!table_device || n_tensors <= 0) return fail(FD_ERR_INVALID, "null/empty tensor table");
    static_assert(sizeof(fd_sgd_tensor) == sizeof(fd_sgd_rec), "table record layout");
    (void)total_numel;
    FD_LAUNCH(fd_sgd_f32, dim3(64, n_tensors), dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const fd_sgd_rec *>(table_device), n_tensors,
              lr, momentum, weight_decay, grad_scale, first_step);
    return check_launch("fd_sgd_f32");
}

}  // extern "C"
