// fd_kernels_io.h -- input preparation on the device: the reference's NYU validation transform
// (dataloaders/nyu.py:48-59: Resize(250/480) -> CenterCrop(228, 304) -> Resize(output_size), all nearest-neighbour, then /255)
// is a pure index map, so the host composes the three steps into one row table and one column table
// (fast-depth_amd/dataloaders/nyu.py) and this kernel gathers: raw HWC uint8 frames + raw depth -> the network's NCHW fp32 input
// (+ the transformed depth target).  At 35 k frames/s the CPU transform (PIL per frame) would be the bottleneck.
#pragma once
#include "fd_device.h"
#include "../../include/fastdepth_hip.h"
#include "fd_viridis.h"

static __global__ void __launch_bounds__(256)
fd_val_transform_u8(const unsigned char *__restrict__ rgb, const float *__restrict__ depth, const int *__restrict__ ymap,
                    const int *__restrict__ xmap, float *__restrict__ x, float *__restrict__ d, int n, int H, int W, int oh, int ow)
{
    const long total = (long)n * oh * ow;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % ow);
        const long t = i / ow;
        const int oy = (int)(t % oh), f = (int)(t / oh);
        const long src = ((long)f * H + ymap[oy]) * W + xmap[ox];
        const unsigned char *p = rgb + src * 3;
        // the reference divides in float64 (np.asfarray(rgb) / 255) and converts to float32 afterwards (dataloader.py:97-99)
        float *o = x + ((long)f * 3 * oh + oy) * ow + ox;
        o[0] = (float)((double)p[0] / 255.0);
        o[(long)oh * ow] = (float)((double)p[1] / 255.0);
        o[2L * oh * ow] = (float)((double)p[2] / 255.0);
        if (d) d[i] = depth[src];
    }
}

// ---- training augmentation (reference dataloaders/nyu.py:26-46 train_transform + transforms.py ColorJitter): per frame a random scale s, rotation and
// flip through Resize(250/480) -> Rotate -> Resize(s) -> CenterCrop(228, 304) -> flip -> Resize(output), every step nearest-neighbour, then brightness /
// contrast / saturation in a random order.  The geometry is again one index map, but a per-frame one with a rotation in the middle:
//     output (oy, ox) --ytab / xtab (last resize, flip, crop, Resize(s) composed)--> (ya, xa) in the rotated 250 x 333 image
//                     --rotation, in double exactly as scipy.ndimage evaluates it--> (iy, ix) in the 250 x 333 image, or outside --> 0
//                     --y1 / x1 (first resize)--> raw frame.
// Three launches: fd_aug_tables (one lane per sequential table: PIL accumulates the source coordinate by repeated addition in double, so a table is sequential);
// fd_aug_gather (geometry ONCE: writes the depth target, applies the colour ops that precede contrast, stashes the uint8 pixel in scratch and adds the
// frame's luma sum -- contrast blends with the mean luma of the WHOLE frame, an exact integer reduction); fd_aug_apply (elementwise on the stash:
// contrast and what follows it, then / 255 -> NCHW).  PIL blends in float32, rounding the product and the sum separately, and SciPy rounds every
// product and sum of the rotation in double: contraction into FMA is switched off wherever that arithmetic is restated.
#define FD_AUG_CROP_H 228
#define FD_AUG_CROP_W 304
#define FD_AUG_MAX_SCALE 4.0     /* bounds the Resize(s) tables (LDS of fd_aug_tables); the reference draws s from [1, 1.5] */
#define FD_AUG_MAX_H1 256        /* capacity of the first resize's tables in scratch: h1 = int(H * (250 / H)) <= 250 */
#define FD_AUG_MAX_W1 1024       /* w1 = int(W * (250 / H)): frames up to 4 : 1 */
#define FD_AUG_PIX_PER_ITEM 8    /* fd_aug_gather: pixels per work-item (a wave's luma partial stays < 2^24: exact in the float shuffles) */

// one frame's derived state in scratch (128 bytes: the luma sums of two frames never share a line)
struct fd_aug_frame {
    double c, s, off_y, off_x;   // rotation: src_y = (off_y + ya * c) + xa * s;  src_x = (off_x + ya * (-s)) + xa * c
    long long luma;              // sum over the frame of the pixels' luma when contrast's turn comes
    float alpha[3];              // blend factor of brightness, contrast, saturation
    float scale;                 // s as float32: depth / s
    int order[3];
    int ok;                      // 0: the record was refused (fd_aug_record_check); the frame comes out as zeros
    int pad[14];
};
static_assert(sizeof(fd_aug_frame) == 128, "the scratch layout of fd_train_transform counts on 128-byte frame headers");
static_assert(sizeof(fd_aug_params) == 48, "fd_aug_params is a 48-byte record on both sides of the C ABI (dataloaders/nyu.py: AUG_DTYPE)");
// The three kernels below are written for 64-lane waves in workgroups of 256 (gfx950, like the rest of the library): fd_aug_tables hands one
// sequential table to lane 0 of each of the FOUR waves, fd_aug_gather reduces over 64 lanes and then over part[4].
#define FD_AUG_WAVE 64
#define FD_AUG_GROUP 256
static_assert(FD_AUG_GROUP == 4 * FD_AUG_WAVE, "fd_aug_tables needs four waves (four sequential tables), fd_aug_gather sums part[4]");

// 0: usable; 1: order is no permutation of {0, 1, 2}; 2: s is not a finite value in (0, FD_AUG_MAX_SCALE]; 3: the image resized by s is smaller than the crop;
// 4: a colour factor or the angle is not finite (a NaN blend has no uint8 value).
// Host (records the host can read) and device (every record: nothing below indexes a table with an unchecked record) apply the same rule.
__host__ __device__ inline int fd_aug_record_check(const fd_aug_params &p, int h1, int w1)
{
    const int o0 = p.order[0], o1 = p.order[1], o2 = p.order[2];
    if (o0 < 0 || o0 > 2 || o1 < 0 || o1 > 2 || o2 < 0 || o2 > 2 || o0 == o1 || o0 == o2 || o1 == o2) return 1;
    if (!(p.s > 0.0 && p.s <= FD_AUG_MAX_SCALE)) return 2;
    if ((int)(h1 * p.s) < FD_AUG_CROP_H || (int)(w1 * p.s) < FD_AUG_CROP_W) return 3;
    const float fmax = 3.402823466e+38f;
    if (!(p.brightness >= -fmax && p.brightness <= fmax) || !(p.contrast >= -fmax && p.contrast <= fmax) || !(p.saturation >= -fmax && p.saturation <= fmax) ||
        !(p.angle >= -1.0e300 && p.angle <= 1.0e300)) return 4;
    return 0;
}

// PIL's NEAREST table of n_in samples resized to n_out: the source coordinate is accumulated by repeated addition in double (the sum PIL forms, not
// i * scale) and truncated.  Sequential, and free of loads: the stores do not stall the chain.
__device__ inline void fd_aug_nearest(int *tab, int n_in, int n_out)
{
    const double scale = (double)n_in / (double)n_out;
    double pos = scale * 0.5;
    for (int i = 0; i < n_out; ++i) {
        const int v = (int)pos;
        tab[i] = v < n_in - 1 ? v : n_in - 1;
        pos += scale;
    }
}

// grid n + 1 workgroups of 256.  Workgroup f < n builds frame f's tables: lane 0 of each of the four waves runs one sequential table -- Resize(s) for
// rows and for columns into LDS (at most FD_AUG_MAX_SCALE * FD_AUG_MAX_H1 / _W1 entries), the last resize for rows and for columns into ytab / xtab --
// and wave 0's lane 1 the rotation and the header; after the barrier all 256 work-items compose: tab[k] = resize_s[crop offset + (flipped) tab[k]].
// Workgroup n builds the first resize's tables, which all frames share.  ytab / xtab are not __restrict__: one lane writes an entry, another rewrites it.
static __global__ void __launch_bounds__(256)
fd_aug_tables(const fd_aug_params *__restrict__ params, fd_aug_frame *__restrict__ frames, int *__restrict__ y1, int *__restrict__ x1,
              int *ytab, int *xtab, int n, int H, int W, int h1, int w1, int oh, int ow)
{
    __shared__ int rs_y[(int)FD_AUG_MAX_SCALE * FD_AUG_MAX_H1], rs_x[(int)FD_AUG_MAX_SCALE * FD_AUG_MAX_W1];
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x, task = (tid % FD_AUG_WAVE) == 0 ? tid / FD_AUG_WAVE : (tid == 1 ? 4 : -1);
    if (f == n) {
        if (task == 0) fd_aug_nearest(y1, H, h1);
        if (task == 1) fd_aug_nearest(x1, W, w1);
        return;
    }
    const fd_aug_params p = params[f];
    const bool ok = fd_aug_record_check(p, h1, w1) == 0;
    const int h2 = ok ? (int)(h1 * p.s) : 0, w2 = ok ? (int)(w1 * p.s) : 0;   // scipy.misc.imresize with a float: (size * s).astype(int); <= the LDS tables by the check
    int *ty = ytab + (long)f * oh, *tx = xtab + (long)f * ow;
    if (ok && task == 0) fd_aug_nearest(rs_y, h1, h2);
    if (ok && task == 1) fd_aug_nearest(rs_x, w1, w2);
    if (ok && task == 2) fd_aug_nearest(ty, FD_AUG_CROP_H, oh);
    if (ok && task == 3) fd_aug_nearest(tx, FD_AUG_CROP_W, ow);
    if (task == 4) {
#pragma clang fp contract(off)
        fd_aug_frame fr = {};
        const double a = p.angle * (3.14159265358979323846 / 180.0);
        const double c = cos(a), s = sin(a), cy = (h1 - 1) / 2.0, cx = (w1 - 1) / 2.0;
        fr.c = c; fr.s = s;
        fr.off_y = cy - (c * cy + s * cx);
        fr.off_x = cx - ((-s) * cy + c * cx);
        fr.luma = 0;
        fr.alpha[0] = p.brightness; fr.alpha[1] = p.contrast; fr.alpha[2] = p.saturation;
        fr.scale = (float)p.s;
        for (int k = 0; k < 3; ++k) fr.order[k] = ok ? p.order[k] : k;
        fr.ok = ok ? 1 : 0;
        frames[f] = fr;
    }
    __syncthreads();                          // (the workgroup's own global stores to ytab / xtab are visible to it after the barrier)
    if (!ok) return;
    // CenterCrop: offset int(round((size - crop) / 2.)), Python's round: half to even.  offset + crop <= size, so every index below is inside rs_y / rs_x.
    const int i0 = (int)rint((h2 - FD_AUG_CROP_H) / 2.0), j0 = (int)rint((w2 - FD_AUG_CROP_W) / 2.0);
    for (int k = tid; k < oh; k += FD_AUG_GROUP) ty[k] = rs_y[i0 + ty[k]];
    for (int k = tid; k < ow; k += FD_AUG_GROUP) tx[k] = rs_x[j0 + (p.flip ? FD_AUG_CROP_W - 1 - tx[k] : tx[k])];
}

// PIL's blend of two uint8 values: deg + alpha * (v - deg) in float32, clipped and truncated.  (For 0 <= alpha <= 1 PIL skips the clip and only
// truncates; the value then lies between deg and v, where the clip changes nothing.)
__device__ __forceinline__ int fd_aug_blend(int deg, int v, float alpha)
{
#pragma clang fp contract(off)
    const float prod = alpha * (float)(v - deg);
    const float t = (float)deg + prod;
    return !(t > 0.0f) ? 0 : (t >= 255.0f ? 255 : (int)t);       // (written so that a NaN, which a checked record cannot produce, still lands inside 0..255)
}
__device__ __forceinline__ int fd_aug_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }      // PIL's RGB -> L
// op 0 brightness (blend with black), 1 contrast (with the frame's mean luma m), 2 saturation (with the pixel's own luma)
__device__ __forceinline__ void fd_aug_color_op(int op, float alpha, int m, int &r, int &g, int &b)
{
    const int deg = op == 0 ? 0 : (op == 1 ? m : fd_aug_luma(r, g, b));
    r = fd_aug_blend(deg, r, alpha); g = fd_aug_blend(deg, g, alpha); b = fd_aug_blend(deg, b, alpha);
}
// (field by field and by selects: a by-value copy of the header, or alpha[op], would live in scratch memory)
__device__ __forceinline__ float fd_aug_alpha(const fd_aug_frame *fr, int op) { return op == 0 ? fr->alpha[0] : (op == 1 ? fr->alpha[1] : fr->alpha[2]); }

// grid (ceil(oh * ow / (256 * FD_AUG_PIX_PER_ITEM)), n)
static __global__ void __launch_bounds__(256)
fd_aug_gather(const unsigned char *__restrict__ rgb, const float *__restrict__ depth, fd_aug_frame *__restrict__ frames, const int *__restrict__ y1,
              const int *__restrict__ x1, const int *__restrict__ ytab, const int *__restrict__ xtab, unsigned *__restrict__ stash,
              float *__restrict__ d, int H, int W, int h1, int w1, int oh, int ow)
{
    __shared__ float part[4];
    const int f = (int)blockIdx.y, px = oh * ow;
    const fd_aug_frame *fr = frames + f;
    const double rc = fr->c, rs = fr->s, off_y = fr->off_y, off_x = fr->off_x;
    const float scale = fr->scale;
    const bool ok = fr->ok != 0;
    const int *yt = ytab + (long)f * oh, *xt = xtab + (long)f * ow;
    const double ymax = (double)(h1 - 1), xmax = (double)(w1 - 1);
    const int o0 = fr->order[0], o1 = fr->order[1], first = o0 == 1 ? 0 : (o1 == 1 ? 1 : 2);
    const float a0 = fd_aug_alpha(fr, o0), a1 = fd_aug_alpha(fr, o1);
    int lsum = 0;
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < px; i += (int)gridDim.x * 256) {
        const int oy = i / ow, ox = i - oy * ow;
        long src = -1;
        if (ok) {
#pragma clang fp contract(off)
            const double ya = (double)yt[oy], xa = (double)xt[ox];
            const double py = ya * rc, qy = xa * rs, px_ = ya * (-rs), qx = xa * rc;
            const double sy = (off_y + py) + qy, sx = (off_x + px_) + qx;
            // scipy.ndimage, mode='constant': inside iff the coordinate lies in [0, n - 1]; then the sample at floor(coordinate + 0.5), which is <= n - 1
            if (sy >= 0.0 && sy <= ymax && sx >= 0.0 && sx <= xmax)
                src = ((long)f * H + y1[(int)floor(sy + 0.5)]) * W + x1[(int)floor(sx + 0.5)];
        }
        int r = 0, g = 0, b = 0;
        if (src >= 0) { const unsigned char *p = rgb + src * 3; r = p[0]; g = p[1]; b = p[2]; }
        if (first > 0) fd_aug_color_op(o0, a0, 0, r, g, b);                            // the ops before contrast's turn
        if (first > 1) fd_aug_color_op(o1, a1, 0, r, g, b);
        lsum += fd_aug_luma(r, g, b);
        stash[(long)f * px + i] = (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
        if (d) d[(long)f * px + i] = src >= 0 ? depth[src] / scale : 0.0f;          // nyu.py:28: float32 depth / s, an IEEE division
    }
    float v = (float)lsum;                                 // <= 8 * 255 per work-item: integers below 2^24 all the way
    for (int m = FD_AUG_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((threadIdx.x % FD_AUG_WAVE) == 0) part[threadIdx.x / FD_AUG_WAVE] = v;
    __syncthreads();
    if (threadIdx.x == 0) fd_atomic_add_i64(&frames[f].luma, (long long)(part[0] + part[1] + part[2] + part[3]));
}

// grid (ceil(oh * ow / 1024), n)
static __global__ void __launch_bounds__(256)
fd_aug_apply(const fd_aug_frame *__restrict__ frames, const unsigned *__restrict__ stash, float *__restrict__ x, int oh, int ow)
{
    __shared__ float unit[256];
    unit[threadIdx.x] = (float)((double)(int)threadIdx.x / 255.0);        // the reference divides in float64 and converts afterwards, as fd_val_transform_u8 does
    __syncthreads();
    const int f = (int)blockIdx.y, px = oh * ow;
    const fd_aug_frame *fr = frames + f;
    // ImageEnhance.Contrast: int(mean + 0.5) of the luma image, the mean a double quotient of two integers
    const int m = (int)((double)fr->luma / (double)px + 0.5);
    const int o0 = fr->order[0], o1 = fr->order[1], o2 = fr->order[2], first = o0 == 1 ? 0 : (o1 == 1 ? 1 : 2);
    const float a0 = fd_aug_alpha(fr, o0), a1 = fd_aug_alpha(fr, o1), a2 = fd_aug_alpha(fr, o2);
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < px; i += (int)gridDim.x * 256) {
        const unsigned u = stash[(long)f * px + i];
        int r = (int)(u & 255u), g = (int)((u >> 8) & 255u), b = (int)((u >> 16) & 255u);
        if (first == 0) fd_aug_color_op(o0, a0, m, r, g, b);                           // contrast and what follows it
        if (first <= 1) fd_aug_color_op(o1, a1, m, r, g, b);
        fd_aug_color_op(o2, a2, m, r, g, b);
        float *o = x + (long)f * 3 * px + i;
        o[0] = unit[r]; o[px] = unit[g]; o[2L * px] = unit[b];
    }
}

// ---- comparison rows (reference utils.py:37-74 colored_depthmap / merge_into_row / merge_into_row_with_gt, deploy/data/visualize.py:22-31): per frame
// `colour frame | depth map ... ` as uint8 RGB, the depth panels viridis-coloured over the frame's joint range.  The reference goes through
// .cpu().numpy(), matplotlib's Colormap.__call__ (float64 over [H, W, 4]) and np.hstack; the arithmetic that decides a byte is small and fixed:
//     rel = (d - d_min) / (d_max - d_min), t = rel * 256      float32, each operation rounded on its own (no reciprocal, no contraction)
//     NaN -> black; t < 0 -> entry 0; t >= 256 -> entry 255 (t == 256 is matplotlib's "1.0 is inside"); otherwise entry int(t)
//     byte = uint8(255 * viridis[entry][c])                   the table of fd_viridis.h
//     colour frame: uint8(255.0f * x), the product in float32, truncated
// Two launches.  fd_viz_range (skipped when the caller gives the ranges): every workgroup reduces its share of a frame's maps with the NaN-propagating
// IEEE minimum / maximum and stores ONE (min, max) partial in its own scratch slot -- plain stores, nothing to zero, no atomics.  fd_viz_paint finishes a
// frame's partials in its prologue (minimum / maximum are exact, commutative and associative, NaN included: any combination order gives the same
// bits), as the train kernels finish the BatchNorm tables, and paints.
#define FD_VIZ_MAX_PARTS 32          /* workgroups of fd_viz_range per frame, at most: wave 0 of fd_viz_paint finishes them in one shuffle tree */
#define FD_VIZ_PART_ELEMS 4096       /* elements a workgroup of fd_viz_range reduces before a further one is worth its launch */
#define FD_VIZ_STORE4 1              /* fd_viz_paint: three dword stores per work-item (w % 4 == 0, pitch % 4 == 0, canvas 4-byte aligned) */
#define FD_VIZ_LOAD4 2               /* 16-byte loads (w % 4 == 0 and every input plane 16-byte aligned) */
static_assert(FD_VIZ_MAX_PARTS <= 64, "one wave of fd_viz_paint finishes a frame's partials");

__device__ __forceinline__ float fd_viz_min(float a, float b) { return __builtin_elementwise_minimum(a, b); }     // NaN if either is NaN (np.min)
__device__ __forceinline__ float fd_viz_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
// all 64 lanes of the calling wave take part
__device__ __forceinline__ void fd_viz_wave_minmax(float &lo, float &hi)
{
    for (int m = 32; m >= 1; m >>= 1) { lo = fd_viz_min(lo, __shfl_xor(lo, m)); hi = fd_viz_max(hi, __shfl_xor(hi, m)); }
}

// grid (n, parts <= FD_VIZ_MAX_PARTS) -- the frame in x, which has no 65535 limit: partials[f][FD_VIZ_MAX_PARTS][2]; workgroup (g, f) writes slot g of frame f.  px = h * w.
static __global__ void __launch_bounds__(256)
fd_viz_range(const float *__restrict__ m0, const float *__restrict__ m1, const float *__restrict__ m2, float *__restrict__ partials, long px, int load4)
{
    __shared__ float part[2][4];
    const int f = (int)blockIdx.x, g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const long first = (long)g * 256 + tid, step = (long)gridDim.y * 256;
    float lo = __builtin_huge_valf(), hi = -__builtin_huge_valf();
    for (int m = 0; m < 3; ++m) {
        const float *p = m == 0 ? m0 : (m == 1 ? m1 : m2);
        if (!p) break;
        p += (long)f * px;
        if (load4) {
            for (long q = first; q < (px >> 2); q += step) {
                const fd_f32x4 v = fd_ld4(p + 4 * q);
                lo = fd_viz_min(fd_viz_min(lo, v.x), fd_viz_min(fd_viz_min(v.y, v.z), v.w));
                hi = fd_viz_max(fd_viz_max(hi, v.x), fd_viz_max(fd_viz_max(v.y, v.z), v.w));
            }
        } else {
            for (long i = first; i < px; i += step) { const float v = p[i]; lo = fd_viz_min(lo, v); hi = fd_viz_max(hi, v); }
        }
    }
    fd_viz_wave_minmax(lo, hi);
    if ((tid & 63) == 0) { part[0][tid >> 6] = lo; part[1][tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0) {
        float *o = partials + ((long)f * FD_VIZ_MAX_PARTS + g) * 2;
        o[0] = fd_viz_min(fd_viz_min(part[0][0], part[0][1]), fd_viz_min(part[0][2], part[0][3]));
        o[1] = fd_viz_max(fd_viz_max(part[1][0], part[1][1]), fd_viz_max(part[1][2], part[1][3]));
    }
}

// one depth value -> its packed colour (r | g << 8 | b << 16)
__device__ __forceinline__ unsigned fd_viz_colour(const unsigned *lut, float d, float d_min, float span)
{
#pragma clang fp contract(off)
    const float rel = (d - d_min) / span;            // an IEEE division, as NumPy's
    const float t = rel * 256.0f;
    if (t != t) return 0u;                           // matplotlib's "bad": (0, 0, 0)
    return lut[t < 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t)];      // under; [255, 256) truncates to 255, t == 256 and over are 255 too
}
// uint8(double(255.0f * x)): truncated toward zero; saturates outside [0, 256 / 255), NaN -> 0 (the reference's cast is platform-defined there)
__device__ __forceinline__ unsigned fd_viz_u8(float x)
{
    const float v = 255.0f * x;
    return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (unsigned)(int)v);
}

// grid (n, gy).  A work-item paints 4 consecutive pixels of one panel row (fewer at the end of a row whose width is no multiple of 4); consecutive
// work-items follow a canvas row through its panels, so a wave's stores are one contiguous run of 768 bytes.
static __global__ void __launch_bounds__(256)
fd_viz_paint(const float *__restrict__ x, const float *__restrict__ m0, const float *__restrict__ m1, const float *__restrict__ m2,
             const float *__restrict__ range, const float *__restrict__ partials, int parts, unsigned char *__restrict__ canvas, long pitch,
             int h, int w, int k, int flags)
{
    __shared__ unsigned lut[256];
    __shared__ float bounds[2];
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
    lut[tid] = (unsigned)fd_viridis_u8[tid][0] | ((unsigned)fd_viridis_u8[tid][1] << 8) | ((unsigned)fd_viridis_u8[tid][2] << 16);
    if (range) {
        if (tid < 2) bounds[tid] = range[2L * f + tid];
    } else if (tid < 64) {                            // wave 0 finishes the frame's partials
        const float *p = partials + ((long)f * FD_VIZ_MAX_PARTS + tid) * 2;
        float lo = tid < parts ? p[0] : __builtin_huge_valf(), hi = tid < parts ? p[1] : -__builtin_huge_valf();
        fd_viz_wave_minmax(lo, hi);
        if (tid == 0) { bounds[0] = lo; bounds[1] = hi; }
    }
    __syncthreads();
    const float d_min = bounds[0], span = bounds[1] - bounds[0];
    const int panels = k + (x ? 1 : 0), wq = (w + 3) >> 2;
    const long px = (long)h * w, items = (long)h * panels * wq;
    for (long it = (long)blockIdx.y * 256 + tid; it < items; it += (long)gridDim.y * 256) {
        const long rp = it / wq, y = rp / panels;
        const int q = (int)(it - rp * wq), j = (int)(rp - y * panels), x0 = q * 4, cnt = w - x0 < 4 ? w - x0 : 4;
        const int mi = x ? j - 1 : j;                 // -1: the colour frame
        const long at = y * w + x0;
        unsigned c[4] = {0u, 0u, 0u, 0u};
        if (mi < 0) {
            const float *p = x + (long)f * 3 * px + at;
            if (flags & FD_VIZ_LOAD4) {
                const fd_f32x4 r = fd_ld4(p), g = fd_ld4(p + px), b = fd_ld4(p + 2 * px);
                c[0] = fd_viz_u8(r.x) | (fd_viz_u8(g.x) << 8) | (fd_viz_u8(b.x) << 16);
                c[1] = fd_viz_u8(r.y) | (fd_viz_u8(g.y) << 8) | (fd_viz_u8(b.y) << 16);
                c[2] = fd_viz_u8(r.z) | (fd_viz_u8(g.z) << 8) | (fd_viz_u8(b.z) << 16);
                c[3] = fd_viz_u8(r.w) | (fd_viz_u8(g.w) << 8) | (fd_viz_u8(b.w) << 16);
            } else {
                for (int e = 0; e < cnt; ++e) c[e] = fd_viz_u8(p[e]) | (fd_viz_u8(p[px + e]) << 8) | (fd_viz_u8(p[2 * px + e]) << 16);
            }
        } else {
            const float *p = (mi == 0 ? m0 : (mi == 1 ? m1 : m2)) + (long)f * px + at;
            if (flags & FD_VIZ_LOAD4) {
                const fd_f32x4 d = fd_ld4(p);
                c[0] = fd_viz_colour(lut, d.x, d_min, span); c[1] = fd_viz_colour(lut, d.y, d_min, span);
                c[2] = fd_viz_colour(lut, d.z, d_min, span); c[3] = fd_viz_colour(lut, d.w, d_min, span);
            } else {
                for (int e = 0; e < cnt; ++e) c[e] = fd_viz_colour(lut, p[e], d_min, span);
            }
        }
        unsigned char *o = canvas + ((long)f * h + y) * pitch + ((long)j * w + x0) * 3;
        if (flags & FD_VIZ_STORE4) {                  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            unsigned *o4 = reinterpret_cast<unsigned *>(o);
            o4[0] = c[0] | (c[1] << 24);
            o4[1] = (c[1] >> 8) | (c[2] << 16);
            o4[2] = (c[2] >> 16) | (c[3] << 8);
        } else {
            for (int e = 0; e < cnt; ++e) {
                o[3 * e] = (unsigned char)(c[e] & 255u); o[3 * e + 1] = (unsigned char)((c[e] >> 8) & 255u); o[3 * e + 2] = (unsigned char)(c[e] >> 16);
            }
        }
    }
}

// ---- gradient exchange in 16 bits (optional: SURVEY.md 8(e), the 7.92 MB form of the data-parallel all-reduce): a bucket of the flat fp32
// gradient vector -> bfloat16 (round to nearest even) before the collective, and back after it.  4 elements per work-item.
static __global__ void __launch_bounds__(256)
fd_cast_f32_bf16(const float *__restrict__ src, fd_bf16 *__restrict__ dst, long n4, long n)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) fd_st4(dst + 4 * i, fd_ld4(src + 4 * i));
    for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) fd_st1(dst + i, src[i]);
}
static __global__ void __launch_bounds__(256)
fd_cast_bf16_f32(const fd_bf16 *__restrict__ src, float *__restrict__ dst, long n4, long n)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) fd_st4(dst + 4 * i, fd_ld4(src + 4 * i));
    for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = fd_ld1(src + i);
}

