"""Numerics of the split-bf16 form of fd_pw_gemm16_f32 (csrc/fd_kernels_gemm16_x3.h) on the CPU.  Measurement aid, no GPU.
usage: python tools/x3_numerics.py [--m 256] [--n 256] [--seed 0]

An fp32 number is the exact sum of three bf16 numbers; six of the nine partial products of a * w carry relative weight >= 2^-16.  This script compares,
against the fp64 product, with  max|y - y64| / max|y64|  as the error:
  fp32   the order of fd_pw_gemm16_f32: two k-halves of every 32-deep K tile, each accumulated in chunks of k = 4 (one v_mfma_f32_16x16x4_f32), added once
  six    the six-product split: a_hi {w_hi, w_mid, w_lo} in one accumulator, a_mid {w_hi, w_mid} + a_lo w_hi in another (the two waves of a SIMD), each
         32-deep tile product formed exactly (fp64) and added with ONE fp32 rounding per MFMA, the two accumulators added once
  three  a_hi w_hi + a_hi w_mid + a_mid w_hi only (NOT what the kernel does: shown for contrast)
and the same through a chain of eleven 512 x 512 layers with ReLU6.  Activations are split by round-to-nearest, weights by truncation (as the kernels do)."""
import argparse

import numpy as np


def bf16_rne(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_trunc(x):
    return (x.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split(x, cut):
    hi = cut(x); r = (x - hi).astype(np.float32)
    mid = cut(r); lo = cut((r - mid).astype(np.float32))
    return hi, mid, lo


def gemm_fp32_order(a, w):
    """two k-halves per 32-deep tile, chunks of 4: every chunk's 4 products are summed exactly and added with one fp32 rounding"""
    m, k = a.shape
    acc = [np.zeros((m, w.shape[0]), np.float32), np.zeros((m, w.shape[0]), np.float32)]
    for t in range(0, k, 32):
        for h in range(2):
            for c in range(t + 16 * h, t + 16 * h + 16, 4):
                acc[h] = (acc[h].astype(np.float64) + a[:, c:c + 4].astype(np.float64) @ w[:, c:c + 4].astype(np.float64).T).astype(np.float32)
    return acc[0] + acc[1]


def gemm_split(a, w, products):
    """products: two lists of (a part, w part) index pairs, one per accumulator; a 32-deep tile product is exact, one fp32 rounding per MFMA"""
    ap, wp = split(a, bf16_rne), split(w, bf16_trunc)
    m, k = a.shape
    accs = []
    for plist in products:
        acc = np.zeros((m, w.shape[0]), np.float32)
        for t in range(0, k, 32):
            for i, j in plist:
                acc = (acc.astype(np.float64) + ap[i][:, t:t + 32].astype(np.float64) @ wp[j][:, t:t + 32].astype(np.float64).T).astype(np.float32)
        accs.append(acc)
    return accs[0] + accs[1]


SIX = [[(0, 0), (0, 1), (0, 2)], [(1, 0), (1, 1), (2, 0)]]
THREE = [[(0, 0), (0, 1)], [(1, 0)]]


def err(y, y64):
    return float(np.abs(y.astype(np.float64) - y64).max() / np.abs(y64).max())


if __name__ == "__main__":
    ap = argparse.ArgumentParser(); ap.add_argument("--m", type=int, default=256); ap.add_argument("--n", type=int, default=256); ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    print("%6s %10s %10s %10s" % ("K", "fp32", "six", "three"))
    for k in (256, 512, 1024):
        a = np.clip(rng.normal(1.0, 2.0, (args.m, k)), 0, 6).astype(np.float32)          # ReLU6-like
        w = (rng.normal(0, 1, (args.n, k)) / np.sqrt(k)).astype(np.float32)
        y64 = a.astype(np.float64) @ w.astype(np.float64).T
        print("%6d %10.2e %10.2e %10.2e" % (k, err(gemm_fp32_order(a, w), y64), err(gemm_split(a, w, SIX), y64), err(gemm_split(a, w, THREE), y64)))
    # a chain of eleven 512 x 512 layers with ReLU6, against fp64 and against the sequential order of the 32x32x2 kernel (k = 2 chunks, one accumulator)
    k = 512
    ws = [(rng.normal(0, 1, (k, k)) * np.sqrt(2.0 / k)).astype(np.float32) for _ in range(11)]
    x0 = np.clip(rng.normal(1.0, 2.0, (args.m, k)), 0, 6).astype(np.float32)

    def seq2(a, w):
        acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
        for c in range(0, a.shape[1], 2):
            acc = (acc.astype(np.float64) + a[:, c:c + 2].astype(np.float64) @ w[:, c:c + 2].astype(np.float64).T).astype(np.float32)
        return acc

    def chain(f, dt):
        x = x0.astype(dt)
        for w in ws:
            x = np.clip(f(x, w), 0, 6).astype(dt)
        return x
    y64 = chain(lambda a, w: a @ w.astype(np.float64).T, np.float64)
    yf, ys, yq = chain(gemm_fp32_order, np.float32), chain(lambda a, w: gemm_split(a, w, SIX), np.float32), chain(seq2, np.float32)
    print("chain of 11 layers:  fp32 order vs fp64 %.2e | six-product vs fp64 %.2e | fp32 order vs sequential 32x32x2 order %.2e | six-product vs sequential %.2e" % (
        err(yf, y64), err(ys, y64), err(yf, yq.astype(np.float64)), err(ys, yq.astype(np.float64))))
