// The arithmetic of gradient accumulation over a window of micro-batches (include/fpd_amd.h, fpd_grad_accum_t), in the
// operation order of the numpy restatement (tests/_accum_ref.py):
//   FIRST  acc  = g                           a copy of the bits: acc is not read
//   ADD    acc  = acc + g                     one float32 addition
//   FIN    g    = acc * s                     one float32 multiplication, s = (float)(1 / m) for a window of m micro-batches
// Each function holds one operation, so there is no multiply-add for a compiler to fuse.
// Host and device compile the same text, so a host build is checked against numpy bit for bit without a GPU
// (tests/test_accum_cpu.py).
#pragma once
#include <stdint.h>

#if !defined(FPD_HD)
#if defined(__HIPCC__)
#define FPD_HD __host__ __device__
#else
#define FPD_HD
#endif
#endif

FPD_HD static inline float fpd_accum_first(float g) { return g; }

FPD_HD static inline float fpd_accum_add(float acc, float g) { return acc + g; }

FPD_HD static inline float fpd_accum_fin(float acc, float s) { return acc * s; }
