// row_ops.h — what the text encoders' kernels (t5.hip, clip.hip) share besides attention: the row prologue of their norms, the
// embedding gather with or without a position table, and the in-place element-wise pass.
#pragma once
#include <stdio.h>
#include "common.h"

// Norms with one wave per row (4 rows per workgroup): x / y of this wave's row.  false: no such row, or a row at or past its sample's
// row_len, which is written as zeros here and not read.
template <typename TI, typename TO, typename P>
__device__ __forceinline__ bool norm_row(const P& p, int lane, const TI*& x, TO*& y) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.rows) return false;
  x = reinterpret_cast<const TI*>(p.x) + (size_t)row * p.C;
  y = reinterpret_cast<TO*>(p.y) + (size_t)row * p.C;
  if (p.row_len) {
    const int smp = (int)(row / p.rows_per_sample), r = (int)(row - (long long)smp * p.rows_per_sample);
    if (r >= p.row_len[smp]) {
      for (int c = lane; c < p.C; c += 64) y[c] = Elem<TO>::from_f(0.f);
      return false;
    }
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// out[r, :] = table[ids[r], :] (+ pos[r % L, :] with POS: one fp32 add, one rounding) in out_dtype; one workgroup per row.  An id outside
// [0, vocab) is clamped (the host validates ids where they enter; the kernel only makes sure that nothing outside the table is read).
template <typename TO, bool POS>
__global__ __launch_bounds__(256) void embed_rows_kernel(const dc_embed_rows_pos_params p) {
  const int r = blockIdx.x;
  long long id = p.ids[r];
  id = id < 0 ? 0 : (id >= p.vocab ? p.vocab - 1 : id);
  const float* src = p.table + (size_t)id * p.C;
  const float* ps = POS ? p.pos + (size_t)(r % p.L) * p.C : nullptr;
  TO* dst = reinterpret_cast<TO*>(p.out) + (size_t)r * p.C;
  for (int c = threadIdx.x; c < p.C; c += 256) dst[c] = Elem<TO>::from_f(POS ? src[c] + ps[c] : src[c]);
}

// dc_embed_rows (POS = false: p.pos and p.L are not looked at) and dc_embed_rows_pos
template <bool POS>
static int embed_rows_launch(const dc_embed_rows_pos_params& p, dc_stream stream, const char* fn) {
  DC_REQUIRE(p.table && (!POS || p.pos) && p.ids && p.out, DC_ERR_ARG, "%s: null pointer", fn);
  DC_REQUIRE((unsigned)p.out_dtype <= DC_F16, DC_ERR_DTYPE, "%s: out_dtype %d", fn, p.out_dtype);
  if (POS) DC_REQUIRE(p.rows > 0 && p.C > 0 && p.vocab > 0 && p.L > 0, DC_ERR_SHAPE, "%s: rows=%d C=%d vocab=%d L=%d", fn, p.rows, p.C, p.vocab, p.L);
  else DC_REQUIRE(p.rows > 0 && p.C > 0 && p.vocab > 0, DC_ERR_SHAPE, "%s: rows=%d C=%d vocab=%d", fn, p.rows, p.C, p.vocab);
  DC_REQUIRE((((uintptr_t)p.table | (POS ? (uintptr_t)p.pos : 0)) & 3) == 0 && (((uintptr_t)p.ids) & 7) == 0 &&
             (((uintptr_t)p.out) & (dc_dtype_size(p.out_dtype) - 1)) == 0, DC_ERR_ALIGN, "%s: pointers must be element aligned", fn);
  char what[40];
  snprintf(what, sizeof(what), "%s: out_dtype", fn);
  return dc_by_dtype(p.out_dtype, what, [&](auto to) {
    hipLaunchKernelGGL((embed_rows_kernel<decltype(to), POS>), dim3((unsigned)p.rows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
    return dc_check_launch(fn);
  });
}

// ------------------------------------------------------------------------------------------------
// x[i] = f(x[i]) in place, a 16-byte chunk per thread and step; F maps a STORAGE element to a storage element, so that a pass can hand
// an element back untouched.  The last n % (16 / size) elements go one by one.
template <typename T, typename F>
__global__ __launch_bounds__(256) void inplace_pass_kernel(T* x, long long n) {
  constexpr int EPC = Elem<T>::EPC;
  const long long nch = n / EPC;
  const long long stride = (long long)gridDim.x * 256;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < nch; c += stride) {
    typename Elem<T>::vec v = *reinterpret_cast<const typename Elem<T>::vec*>(x + c * EPC);
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[e] = F::template run<T>(v[e]);
    *reinterpret_cast<typename Elem<T>::vec*>(x + c * EPC) = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - nch * EPC)) {
    T* t = x + nch * EPC + threadIdx.x;
    *t = F::template run<T>(*t);
  }
}

// dc_relu / dc_act_pass: the checks on (x, n, dtype), the grid, and launch(t, nb, stream) with a value of the element type
template <typename L>
static int inplace_pass_launch(void* x, long long n, int dtype, dc_stream stream, const char* fn, L&& launch) {
  DC_REQUIRE((unsigned)dtype <= DC_F16, DC_ERR_DTYPE, "%s: dtype %d", fn, dtype);
  DC_REQUIRE(n > 0, DC_ERR_SHAPE, "%s: n=%lld", fn, n);
  DC_REQUIRE((((uintptr_t)x) & 15) == 0, DC_ERR_ALIGN, "%s: x must be 16-byte aligned", fn);
  const long long nch = n / (16 / dc_dtype_size(dtype));
  long long nb = (nch + 255) / 256;
  nb = nb < 1 ? 1 : (nb > 4096 ? 4096 : nb);
  char what[40];
  snprintf(what, sizeof(what), "%s: dtype", fn);
  return dc_by_dtype(dtype, what, [&](auto t) {
    launch(t, dim3((unsigned)nb), reinterpret_cast<hipStream_t>(stream));
    return dc_check_launch(fn);
  });
}
