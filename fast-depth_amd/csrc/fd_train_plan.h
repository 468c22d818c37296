// fd_train_plan.h -- the train plan's records (TLayer, fd_train_plan), build switches and small helpers: shared by the two train translation units
// (fd_train_fwd.hip: plan creation + train-mode forward, fd_train_impl.h; fd_train_bwd.hip: backward, loss, SGD, gradient exchange, fd_train_bwd_impl.h).
//
// Workspace layout of a train plan:
//   [z_i]   raw conv output of every unit, NHWC, fp32 or bf16 (plan dtype), all kept (they are the saved tensors of backward)
//   [st_i]  per-unit BatchNorm table [4][C]: scale, shift, mean, invstd (written by the unit's finalising workgroup: fd_bn_publish)
//   [stat]  per-unit BatchNorm statistics rows, forward (sum z, sum z^2) and backward (sum G, sum G*xhat): int64 [nr][3 bins][2][C] each (fd_device.h:
//           fd_stat_add / fd_stat_total), ONE contiguous region zeroed by a single memset at the start of every forward
//   backward only: [g_a, g_b] ping-pong dLoss/d(BN output) buffers, [skipgrad_k] decoder->skip gradient buffers,
//   [coef_i] per-unit BN-backward coefficient tables, [wpart_i] per-unit weight-gradient partials (reduced by ONE launch per backward
//   range: fd_reduce_weights_batch_f32).
//   bf16 plans: [wt_i, wtt_i] the 16-bit operand copies of every pointwise weight (re-made from the fp32 masters each step).
#pragma once
#include <type_traits>
#include "fd_kernels_train.h"
#include "fd_kernels_bwd.h"
#include "fd_kernels_train_h16.h"
#include "fd_kernels_io.h"

// workgroups the pointwise weight-gradient GEMM aims for (output tiles x pixel splits); every split writes a private fp32 partial
// tile that fd_reduce_partials_f32 sums afterwards, so more splits = more parallelism but more partial traffic
// (measured at batch 32: 2048 is best for the fp32 kernel; the bf16 one, whose MFMA part is 16x shorter, wants fewer)
// tile shapes of the 5x5 depthwise train kernels (build switches for tools/build_variant.py sweeps; the defaults are the measured best)
#ifndef FD_T_DW5_FTH
#define FD_T_DW5_FTH 8      // forward: rows (balanced over the map), columns
#define FD_T_DW5_FTW 16
#define FD_T_DW5_WTH 8      // backward-weights: output-space tile
#define FD_T_DW5_WTW 16
#define FD_T_DW5_DTH 8      // backward-data: input-space tile
#define FD_T_DW5_DTW 16
#endif
#ifndef FD_T_S2_DTH
#define FD_T_S2_DTH 8       // stride-2 units (single-staging backward kernel): input-space tile
#define FD_T_S2_DTW 16
#endif
#ifndef FD_DW_WGRAD_TARGET_WGS
#define FD_DW_WGRAD_TARGET_WGS 1536   // depthwise weight-gradient kernel: a workgroup walks up to a tile row's tiles as long as about this many workgroups remain
#endif
#ifndef FD_WGRAD_TUNE_H16
#define FD_WGRAD_TUNE_H16 640      // (round 3, paired launch: 640 -> 2.840 ms per bf16 step, 1024 -> 2.877, 512 -> 2.860; fewer splits = fewer partial bytes)
#endif
#ifndef FD_WGRAD_TARGET_WGS_F32
#define FD_WGRAD_TARGET_WGS_F32 1536   // (round 3, paired launch: 1024 -> 4.355 ms per fp32 step, 1536 -> 4.340, 2048 -> 4.361, 3072 -> 4.364)
#endif
#define FD_WGRAD_TARGET_WGS_H16 (FD_WGRAD_TUNE_H16)

// (a global name, not the anonymous namespace: fd_train_plan below has external linkage and both train translation units must see ONE class type --
// an anonymous-namespace member type makes the two definitions of fd_train_plan different classes, an ODR violation)
struct fd_train_layer {
    fd_layer_desc d;
    int in_h = 0, in_w = 0, out_h = 0, out_w = 0;   // in_* = logical (post-upsample) input size; head: out_* = LOW-res size when upsample
    bool head = false;
    int mode = 0;
    int csplit = 0;                  // concatenating depthwise consumer (mode 3): channels [0, csplit) come from src, the rest from skip
    int cbq = 0, th = 0, tw = 0, tiles_x = 0, tiles_y = 0;   // dw tiling (forward kernel)
    int dw_n = 4;                                             // channels per work-item of the LDS-tiled depthwise kernels (8: bf16 plans, storage-typed LDS patches; fd_lane)
    int bth = 0, btw = 0;                                     // output-space tile of the backward-weights kernel
    // depthwise forward form: fd_dwconv_train (LDS-tiled) / fd_dw3_rows_train (register window) / fd_dw3_rows_fwd / fd_dw5_rows_train (16-bit plans: row-walking)
    enum class DwFwd { TILED, REGWIN, ROWS3, ROWS5 } fwd = DwFwd::TILED;
    int rows_th = 0;                                          // REGWIN: row-strip height
    int rows_cl = 0, rows_groups = 0, rows_bh = 0;            // ROWS3 / ROWS5: channel lanes per strip (ROWS3), strip groups per row, output rows per band
    int stemw_groups = 0, stemw_bh = 0;                       // > 0: the stem's backward weights run on fd_stem_wgrad_rows (16-bit plans): column groups per row, rows per band
    // depthwise backward form (dw_bwd_plan, fd_train_impl.h): fd_dw5_bwd_rows / fd_dw3_bwd_rows / fd_dw3s2_bwd_rows / fd_dw3s2_dgrad_rows + fd_dw3_wgrad_rows /
    // fd_dw_bwd1 / fd_dw_bwd / fd_dw_wgrad + fd_dw_dgrad
    enum class DwBwd { ROWS5, ROWS3, ROWS3S2, REGWIN_S2, BWD1, PAIR, SEPARATE } bwd = DwBwd::SEPARATE;
    int d_th = 0, d_tw = 0, d_tiles_x = 0, d_gx = 0;          // LDS-tiled backward data (BWD1 / PAIR / SEPARATE): input-space tile, tiles per row / per image
    int w_tiles_x = 0, w_tpw = 0, w_gx = 0;                   // LDS-tiled backward weights: output-space tiles per row, tiles per workgroup, workgroups per image
    int rb_groups = 0, rb_bh = 0, rb_wgs = 0, rb_cl = 0;      // row kernels: column groups per row, rows per band, workgroups per image and role, channel lanes (ROWS3)
    int rw_th_d = 0, rw_th_w = 0;                             // REGWIN_S2: strip heights of fd_dw3s2_dgrad_rows / fd_dw3_wgrad_rows ...
    dim3 rw_grid_d, rw_grid_w;                                // ... and their grids
    size_t blds = 0, blds2 = 0;                               // dynamic LDS: BWD1 / PAIR (+ the in-kernel finalisation's coefficients); SEPARATE: fd_dw_dgrad / fd_dw_wgrad
    long nblk_b = 0;                                          // backward-data workgroups (all images) that deal partials to the producer's backward statistics rows
    int stem_band = 0;                                        // floats of the stem kernels' input band in LDS
    int pstr = 0, bpstr = 0;                                  // LDS patch pitch (floats) of the forward / the backward depthwise kernels
    int chunk = 0;                                            // stem
    int m_tiles = 0, n_tiles = 0, pw_tn = 1;                  // pw (pw_tn: 32-column tiles per wave of the 16-bit forward GEMM)
    int pw16_tm = 0, pw16_stride = 0;                         // fp32 plans: the forward runs on fd_pw_gemm16_f32<TM, ..., TRAIN> (one workgroup per CU, rows in strides of pw16_stride)
    size_t lds = 0;
    dim3 grid;
    int nblk = 0;                    // workgroups per channel of this unit's forward kernel that add a partial sum to its statistics rows
    int nr_cap = 1;                  // statistics rows reserved per direction (stat_nr of the unit's pixel count / 64)
    int nr_f = 1;                    // rows its forward kernel deals its partials to (stat_nr(nblk), <= nr_cap)
    int nr_b = 1;                    // rows the backward kernel of its CONSUMER deals the (sum G, sum G*xhat) partials to (stat_nr of that kernel's nblk_b)
    size_t sf_off = 0, sb_off = 0;   // forward / backward statistics rows
    int bwd_fin_rows = 0;            // > 0: the unit's first backward kernel finalises its BatchNorm backward from these nr_b rows (bwd_fin_candidate)
    bool fin_by_consumer = false;    // this unit's BatchNorm is finalised inside its consumer's forward kernel (no fd_bn_finalize_rows_f32 launch)
    size_t z_off = 0, z_elems = 0;   // raw output
    size_t st_off = 0;               // [4][C] table
    size_t coef_off = 0;             // backward coefficient table [4][C]
    double n_stat = 0, n_unbiased = 0;
    long M = 0;                      // pixels of the stored output (B*out_h*out_w)
    // backward bookkeeping
    int consumer = -1;               // unit that reads this output as `src`
    int skip_consumer = -1;          // decoder unit that reads this output as `skip` (-1: none)
    size_t g_off = 0;                // dLoss/dy buffer of this unit
    size_t sg_off = 0;               // decoder->skip gradient buffer (only for skip sources)
    size_t wt_off = 0, wtt_off = 0;  // 16-bit plans: W as [N][K64] and W^T as [K][N64]
    size_t dz_off = 0;               // 16-bit pointwise units under FD_PLAN_KEEP_ACTIVATIONS: dz kept apart from G (0 = in place)
    size_t wp_off = 0, wp_elems = 0; // this unit's weight-gradient partial rows (reduced by one launch per backward range)
    int k64 = 0, n64 = 0;
};
typedef fd_train_layer TLayer;

struct fd_train_plan {
    std::vector<TLayer> layers;
    int B = 0, H = 0, W = 0, dtype = FD_F32;
    uint32_t flags = 0, tune = 0;    // public plan flags (include/fastdepth_hip.h) / private tuning mask (fd_tuning.h)
    size_t esz = 4;                  // bytes per stored activation / activation-gradient element
    size_t ws_bytes = 0, stat_off = 0, stat_bytes = 0;   // the statistics rows of all units (both directions): zeroed per step
    bool bwd_stats_clean = false;    // the backward rows are still zero (no backward has run since the last forward's memset)
    unsigned char *ws = nullptr;
    bool forward_done = false;
    float eps = 1e-5f;
    const void *x_saved = nullptr;   // the network input of the last forward (the stem's weight gradient re-reads it)
};

namespace {

inline float *tws(fd_train_plan *p, size_t off) { return reinterpret_cast<float *>(p->ws + off); }
template <typename T> inline T *twt(fd_train_plan *p, size_t off) { return reinterpret_cast<T *>(p->ws + off); }

// Statistics rows a producer of `nblk` workgroups per channel deals its partial sums to: one address takes an atomic every ~22 ns (measured,
// tools/microbench/stat_atomics.hip), so an address should see at most ~FD_STAT_ADDS_PER_ROW of them during the producer's life; a power of two
// <= FD_STAT_MAX_ROWS (the consumer adds nr x 3 integers per channel and sum).
#ifndef FD_STAT_ADDS_PER_ROW
#define FD_STAT_ADDS_PER_ROW 128
#endif
// A consumer (or the unit's own first backward kernel) finalises a BatchNorm in its prologue only when the rows are few: every workgroup reads
// nr x 3 bins x 2 sums of 8 bytes per channel.  ALL: kernels whose work-items each finalise whole channels (pointwise GEMMs, the register-window and head
// kernels); BLOCK: kernels that deal a channel's rows to 256 / CB work-items (LDS-tiled depthwise kernels, the 16-bit apply pass).  Units with more rows
// -- the large maps, whose kernels run 20 ... 160 us -- keep a finalisation launch of their own (fd_bn_finalize_rows_f32: 4 us).
#ifndef FD_STAT_FIN_MAX_ROWS_ALL
#define FD_STAT_FIN_MAX_ROWS_ALL 2
#define FD_STAT_FIN_MAX_ROWS_BLOCK 8
#endif
#ifndef FD_PW_BWD_W_FIRST
#define FD_PW_BWD_W_FIRST 1             // paired 16-bit pointwise backward: the (long-lived) weight-gradient workgroups are numbered before the backward-data tiles where they are the fewer
#endif
#ifndef FD_PW_BWD_W_FIRST_F32
#define FD_PW_BWD_W_FIRST_F32 1         // the same numbering in the fp32 paired launch (fd_pw_bwd_f32)
#endif
#ifndef FD_STEMW_BAND
#define FD_STEMW_BAND 14                // output rows per band of fd_stem_wgrad_rows
#endif
#ifndef FD_STEMW_CPL
#define FD_STEMW_CPL 2                  // output channels per lane of fd_stem_wgrad_rows (2 or 4)
#endif
#ifndef FD_STAT_FIN_MAX_ROWS_ROWK
#define FD_STAT_FIN_MAX_ROWS_ROWK 8       // ... the row-walking depthwise kernels (a few hundred fat workgroups per launch; 16 measured slower: DESIGN Appendix A)
#endif
inline int stat_nr(long nblk)
{
    int nr = 1;
    while (nr < FD_STAT_MAX_ROWS && (long)nr * FD_STAT_ADDS_PER_ROW < nblk) nr *= 2;
    return nr;
}
inline int stat_pitch(int C) { return (C + 15) / 16 * 16; }      // channel pitch of a unit's rows: every [row][bin][sum] slot starts its own 128-byte line
inline size_t stat_rows_bytes(int nr, int C) { return ((size_t)nr * FD_STAT_BINS * 2 + 2) * stat_pitch(C) * sizeof(long long); }     // (+ the poison flags: fd_device.h)
inline long long *stat_ptr(fd_train_plan *p, size_t off) { return reinterpret_cast<long long *>(p->ws + off); }
// this unit's forward rows as its producer kernel sees them
inline fd_stat_rows fwd_rows(fd_train_plan *p, const TLayer &L) { return fd_stat_rows{stat_ptr(p, L.sf_off), L.nr_f, stat_pitch(L.d.cout)}; }
// unit u's backward rows as the backward-data kernel of its consumer sees them
inline fd_stat_rows bwd_rows(fd_train_plan *p, int u) { const TLayer &U = p->layers[u]; return fd_stat_rows{stat_ptr(p, U.sb_off), U.nr_b, stat_pitch(U.d.cout)}; }

// calls fn(fd_int<4>) or -- 16-bit storage types only -- fn(fd_int<8>): the lane width (fd_lane) of the LDS-tiled depthwise kernels
template <typename T, typename F> inline void fd_by_lane_width(int n, F &&fn)
{
    if constexpr (!std::is_same<T, float>::value) { if (n == 8) { fn(fd_int<8>{}); return; } }
    fn(fd_int<4>{});
}
// host mirror of fd_lds_patch_bytes (fd_kernels_train.h): bytes of an LDS patch image of npx pixels at pitch pstr in elements of `le` bytes
inline size_t lds_patch_bytes(long npx, int pstr, int le) { return std::max(align_up((size_t)npx * pstr * le, 16), (size_t)8192); }

// ---- the depthwise backward ----
template <int K_, int S_, int MODE_, int ACT1_, int ACT2_, int ADD_SG_> struct fd_dw_inst {
    static constexpr int K = K_, S = S_, MODE = MODE_, ACT1 = ACT1_, ACT2 = ACT2_, ADD_SG = ADD_SG_;
};
// calls fn(fd_dw_inst<...>) with the instance of the single / paired / row-walking backward kernels for depthwise unit i's kernel size / stride / input
// composition / activations (act2: the skip tensor's); false: none (an unusual combination -- sibling / custom plans: the two separate kernels cover it)
template <typename F> inline bool fd_by_dw_instance(const fd_train_plan *p, int i, F &&fn)
{
    const TLayer &L = p->layers[i];
    const TLayer &P = p->layers[L.d.src];
    const int a1 = P.d.act, a2 = L.d.skip >= 0 ? p->layers[L.d.skip].d.act : FD_ACT_RELU6;
    const bool add = P.skip_consumer >= 0 && L.mode == 0;
    switch (L.d.ksize * 100 + L.d.stride * 10 + L.mode) {
    case 310: if (a1 != FD_ACT_RELU6 || add) return false; fn(fd_dw_inst<3, 1, 0, FD_ACT_RELU6_, FD_ACT_RELU6_, 0>{}); return true;
    case 320:
        if (a1 != FD_ACT_RELU6) return false;
        if (add) fn(fd_dw_inst<3, 2, 0, FD_ACT_RELU6_, FD_ACT_RELU6_, 1>{}); else fn(fd_dw_inst<3, 2, 0, FD_ACT_RELU6_, FD_ACT_RELU6_, 0>{});
        return true;
    case 510: if (a1 != FD_ACT_RELU6 || add) return false; fn(fd_dw_inst<5, 1, 0, FD_ACT_RELU6_, FD_ACT_RELU6_, 0>{}); return true;
    case 511: if (a1 != FD_ACT_RELU) return false; fn(fd_dw_inst<5, 1, 1, FD_ACT_RELU_, FD_ACT_RELU6_, 0>{}); return true;
    case 512: if (a1 != FD_ACT_RELU || a2 != FD_ACT_RELU6) return false; fn(fd_dw_inst<5, 1, 2, FD_ACT_RELU_, FD_ACT_RELU6_, 0>{}); return true;
    case 513: if (a1 != FD_ACT_RELU || a2 != FD_ACT_RELU6) return false; fn(fd_dw_inst<5, 1, 3, FD_ACT_RELU_, FD_ACT_RELU6_, 0>{}); return true;
    }
    return false;
}
// the unit's backward runs on a row-walking kernel of fd_kernels_dw5p_bwd.h
inline bool bwd_on_row_kernel(const TLayer &L)
{
    return L.d.op == FD_OP_DW && (L.bwd == TLayer::DwBwd::ROWS5 || L.bwd == TLayer::DwBwd::ROWS3 || L.bwd == TLayer::DwBwd::ROWS3S2);
}

}  // namespace
