// _contrib_FocalLoss and _contrib_BBoxNorm for gfx950 (RetinaNet / RepPoints training head), fp32.
//
// The reference backward (operator_cxx/contrib/focal_loss-inl.h:116-231) materialises seven
// (B, nbox, nclass) temporaries -- positive, negative, one_hot, grad, ignore_index, one_bc and the
// product with ograd -- out of a 1.5-1.8 GB workspace, each an mshadow expression of its own.  The
// whole computation is a function of (out[b,n,c], label[b,n]) and one batch-wide integer, so here it
// is one streaming pass: 8 bytes per element + 4 per row, nothing else touches memory.
//
// Kernels:
//   focal_sigmoid   out = 1 / (1 + exp(-x))                       (mshadow_op::sigmoid, :113)
//   label_count     count = #(label >= 1) over the batch, an int in the workspace (wave reduction on
//                   the VALU, one atomic per workgroup; cleared by a one-lane kernel); both backward
//                   kernels read it from there, so there is no host round trip and the call can be
//                   captured in a graph
//   focal_bwd       the element rule of :186-230 with the reference's operation order in fp32
//                   (no contraction: the library is built with -ffp-contract=off).  One float4 per
//                   lane per trip when nclass % 4 == 0 and the pointers are 16-byte aligned, one
//                   float otherwise.  The two branches share their shape -- coefficient * pow(r, gamma)
//                   * (gamma * q * log(q + eps) +/- ...) with (q, r) = (p, 1 - p) or (1 - p, p) --
//                   so a lane evaluates ONE log and ONE pow on selected operands and a wave with a
//                   positive in it does not run both sides.
//   bbox_norm_bwd   gdata = gout / max(1, count + 1)              (bbox_norm-inl.h:116-126)
#include "common.h"
#include "loss_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {

constexpr int kFlT = 256;
constexpr int kFlMaxBlocks = kNumCU * 8;  // memory-bound grid: 8 workgroups per CU, grid-stride the rest
constexpr long kFlMaxElems = 2147483647L; // element indices, and the label count, are 32-bit inside the kernels

static int fl_grid(long items) {
  const long b = (items + kFlT - 1) / kFlT;
  return (int)(b < 1 ? 1 : b > kFlMaxBlocks ? kFlMaxBlocks : b);
}

template <bool VEC>
__global__ __launch_bounds__(kFlT) void focal_sigmoid_kernel(const float* __restrict__ x,
                                                             float* __restrict__ y, long n) {
  const long step = (long)gridDim.x * kFlT;
  if (VEC) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4* y4 = reinterpret_cast<float4*>(y);
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * kFlT + threadIdx.x; i < n4; i += step) {
      const float4 v = x4[i];
      y4[i] = make_float4(sigmoid_f32(v.x), sigmoid_f32(v.y), sigmoid_f32(v.z), sigmoid_f32(v.w));
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * kFlT + threadIdx.x; i < n; i += step) y[i] = sigmoid_f32(x[i]);
  } else {
    for (long i = (long)blockIdx.x * kFlT + threadIdx.x; i < n; i += step) y[i] = sigmoid_f32(x[i]);
  }
}

__global__ void label_count_clear_kernel(int* __restrict__ count) {
  if (threadIdx.x == 0) *count = 0;
}

// F<le>(1.f, label) summed over the batch (:218-219, bbox_norm-inl.h:119-120)
__global__ __launch_bounds__(kFlT) void label_count_kernel(const float* __restrict__ label, long n,
                                                           int* __restrict__ count) {
  __shared__ int wsum[kFlT / kWave];
  const long step = (long)gridDim.x * kFlT;
  int c = 0;
  for (long i = (long)blockIdx.x * kFlT + threadIdx.x; i < n; i += step) c += 1.0f <= label[i] ? 1 : 0;
  c = wave_sum_i32(c);
  if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kFlT / kWave; ++w) t += wsum[w];
    if (t) atomicAdd(count, t);
  }
}

struct FocalArgs {
  const float* out;
  const float* label;
  const float* ograd;  // null: out_grad=False
  float* gdata;
  const int* count;
  unsigned rows, nclass;
  float alpha, one_minus_alpha, gamma, grad_scale, batch_scale;
  int normalization;
};

// one element of :192-230 before the ograd product; `cls` is int(label - 1) or -1 (no class), ignore = (label == -1)
template <int GAMMA>
__device__ __forceinline__ float focal_elem(const FocalArgs& a, float p, bool pos) {
  const float eps = 1e-14f;
  const float omp = 1.0f - p;
  const float q = pos ? p : omp, r = pos ? omp : p;
  // gamma * q * log(q + eps): (gamma * q) * log(...)
  const float t = (a.gamma * q) * logf(q + eps);
  // positive: t + p - 1; negative: t - p
  const float inner = pos ? (t + p) - 1.0f : t - p;
  const float v = ((pos ? a.alpha : a.one_minus_alpha) * pow_gamma<GAMMA>(r, a.gamma)) * inner;
  return pos ? v : -v;
}

__device__ __forceinline__ float focal_scale(const FocalArgs& a, float g, float norm) {
  if (a.normalization == 2) return (g * a.grad_scale) / norm;
  if (a.normalization == 1) return g * a.batch_scale;
  return g * a.grad_scale;
}

// mxnet_op one_hot: j = static_cast<int>(label - 1); a class only for 0 <= j < nclass
__device__ __forceinline__ int focal_class(float label) {
  const float l = label - 1.0f;
  return l >= -2147483648.0f && l < 2147483648.0f ? (int)l : -1;  // (NaN and out-of-range: no class)
}

template <int GAMMA, bool VEC>
__global__ __launch_bounds__(kFlT) void focal_bwd_kernel(FocalArgs a) {
  const float norm = (float)*a.count + 1.0f;  // temp = sum + 1.f, no max (:220-221)
  const unsigned step = gridDim.x * kFlT;
  if (VEC) {
    const unsigned nc4 = a.nclass >> 2;
    const unsigned items = a.rows * nc4;  // (< 2^31: the entry point's limit; i + step cannot wrap)
    const float4* o4 = reinterpret_cast<const float4*>(a.out);
    const float4* g4 = reinterpret_cast<const float4*>(a.ograd);
    float4* d4 = reinterpret_cast<float4*>(a.gdata);
    for (unsigned i = blockIdx.x * kFlT + threadIdx.x; i < items; i += step) {
      const unsigned row = i / nc4;
      const int c0 = (int)(i - row * nc4) << 2;
      const float lab = a.label[row];
      const float4 p = o4[i];
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lab != -1.0f) {
        const int cls = focal_class(lab);
        g.x = focal_elem<GAMMA>(a, p.x, cls == c0);
        g.y = focal_elem<GAMMA>(a, p.y, cls == c0 + 1);
        g.z = focal_elem<GAMMA>(a, p.z, cls == c0 + 2);
        g.w = focal_elem<GAMMA>(a, p.w, cls == c0 + 3);
      }
      if (g4) {
        const float4 og = g4[i];
        g.x *= og.x; g.y *= og.y; g.z *= og.z; g.w *= og.w;
      }
      d4[i] = make_float4(focal_scale(a, g.x, norm), focal_scale(a, g.y, norm), focal_scale(a, g.z, norm),
                          focal_scale(a, g.w, norm));
    }
  } else {
    const unsigned items = a.rows * a.nclass;
    for (unsigned i = blockIdx.x * kFlT + threadIdx.x; i < items; i += step) {
      const unsigned row = i / a.nclass;
      const int c = (int)(i - row * a.nclass);
      const float lab = a.label[row];
      float g = 0.f;
      if (lab != -1.0f) g = focal_elem<GAMMA>(a, a.out[i], focal_class(lab) == c);
      if (a.ograd) g *= a.ograd[i];
      a.gdata[i] = focal_scale(a, g, norm);
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kFlT) void bbox_norm_bwd_kernel(const float* __restrict__ gout,
                                                             float* __restrict__ gdata, long n,
                                                             const int* __restrict__ count) {
  const float norm = fmaxr(1.0f, (float)*count + 1.0f);
  const long step = (long)gridDim.x * kFlT;
  if (VEC) {
    const float4* s4 = reinterpret_cast<const float4*>(gout);
    float4* d4 = reinterpret_cast<float4*>(gdata);
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * kFlT + threadIdx.x; i < n4; i += step) {
      const float4 v = s4[i];
      d4[i] = make_float4(v.x / norm, v.y / norm, v.z / norm, v.w / norm);
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * kFlT + threadIdx.x; i < n; i += step)
      gdata[i] = gout[i] / norm;
  } else {
    for (long i = (long)blockIdx.x * kFlT + threadIdx.x; i < n; i += step) gdata[i] = gout[i] / norm;
  }
}

static bool aligned16(const void* a, const void* b, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// the batch-wide count lives in the first int of the 256-byte aligned workspace
static int count_labels(const float* label, long n, void* workspace, size_t workspace_bytes,
                        const char* who, int** count, hipStream_t st) {
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  const size_t need = (size_t)(base - (char*)workspace) + sizeof(int);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "%s workspace too small: %zu < %zu bytes", who, workspace_bytes, need);
  *count = reinterpret_cast<int*>(base);
  // (a kernel, not a memset node: a captured graph then holds kernel nodes only, ordered like any other launch)
  hipLaunchKernelGGL(label_count_clear_kernel, dim3(1), dim3(kWave), 0, st, *count);
  hipLaunchKernelGGL(label_count_kernel, dim3(fl_grid(n)), dim3(kFlT), 0, st, label, n, *count);
  return SD_OK;
}

template <bool VEC>
static void launch_focal_bwd(const FocalArgs& a, int grid, hipStream_t st) {
  if (a.gamma == 2.0f)
    hipLaunchKernelGGL((focal_bwd_kernel<2, VEC>), dim3(grid), dim3(kFlT), 0, st, a);
  else if (a.gamma == 1.0f)
    hipLaunchKernelGGL((focal_bwd_kernel<1, VEC>), dim3(grid), dim3(kFlT), 0, st, a);
  else if (a.gamma == 0.0f)
    hipLaunchKernelGGL((focal_bwd_kernel<0, VEC>), dim3(grid), dim3(kFlT), 0, st, a);
  else
    hipLaunchKernelGGL((focal_bwd_kernel<-1, VEC>), dim3(grid), dim3(kFlT), 0, st, a);
}

}  // namespace sd

using namespace sd;

extern "C" int sd_focal_loss_fwd(const float* data, float* out, long n, void* stream) {
  SD_REQUIRE(n >= 0, "n=%ld is negative", n);
  if (n == 0) return SD_OK;
  SD_REQUIRE(data && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (aligned16(data, out))
    hipLaunchKernelGGL(focal_sigmoid_kernel<true>, dim3(fl_grid(n >> 2)), dim3(kFlT), 0, st, data, out, n);
  else
    hipLaunchKernelGGL(focal_sigmoid_kernel<false>, dim3(fl_grid(n)), dim3(kFlT), 0, st, data, out, n);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" size_t sd_focal_loss_workspace_bytes(void) { return 512; }

extern "C" int sd_focal_loss_bwd(const float* out, const float* label, const float* ograd_or_null,
                                 float* gdata, int B, int nbox, int nclass, float alpha, float gamma,
                                 float grad_scale, int normalization, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  SD_REQUIRE(B >= 0 && nbox >= 0 && nclass >= 0, "negative dimension (B=%d nbox=%d nclass=%d)", B, nbox, nclass);
  SD_REQUIRE(normalization >= 0 && normalization <= 2, "normalization=%d outside 0 (null), 1 (batch), 2 (valid)",
             normalization);
  SD_REQUIRE(alpha == alpha && gamma == gamma, "alpha or gamma is NaN");
  const long rows = (long)B * nbox, n = rows * nclass;
  if (n > kFlMaxElems)
    return fail(SD_ERR_UNSUPPORTED, "B*nbox*nclass = %ld elements exceed the limit %ld", n, kFlMaxElems);
  if (rows == 0 || nclass == 0) return SD_OK;
  SD_REQUIRE(out && label && gdata, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  FocalArgs a{};
  int* count = nullptr;
  if (int e = count_labels(label, rows, workspace, workspace_bytes, "focal_loss_bwd", &count, st)) return e;
  a.out = out; a.label = label; a.ograd = ograd_or_null; a.gdata = gdata; a.count = count;
  a.rows = (unsigned)rows; a.nclass = (unsigned)nclass;
  a.alpha = alpha; a.one_minus_alpha = 1.0f - alpha; a.gamma = gamma; a.grad_scale = grad_scale;
  a.batch_scale = grad_scale / (float)B;  // param_.grad_scale / grad.shape_[0] (:227)
  a.normalization = normalization;
  if (nclass % 4 == 0 && aligned16(out, gdata, ograd_or_null))
    launch_focal_bwd<true>(a, fl_grid(n >> 2), st);
  else
    launch_focal_bwd<false>(a, fl_grid(n), st);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_bbox_norm_bwd(const float* gout, const float* label, float* gdata, int B, long n_per_image,
                                long n_label_per_image, void* workspace, size_t workspace_bytes,
                                void* stream) {
  SD_REQUIRE(B >= 0 && n_per_image >= 0 && n_label_per_image >= 0,
             "negative dimension (B=%d n_per_image=%ld n_label_per_image=%ld)", B, n_per_image,
             n_label_per_image);
  const long n = (long)B * n_per_image, nl = (long)B * n_label_per_image;
  if (nl > kFlMaxElems)
    return fail(SD_ERR_UNSUPPORTED, "B*n_label_per_image = %ld labels exceed the limit %ld", nl, kFlMaxElems);
  if (n == 0) return SD_OK;
  SD_REQUIRE(gout && gdata && (label || nl == 0), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  int* count = nullptr;
  if (int e = count_labels(label, nl, workspace, workspace_bytes, "bbox_norm_bwd", &count, st)) return e;
  if (aligned16(gout, gdata))
    hipLaunchKernelGGL(bbox_norm_bwd_kernel<true>, dim3(fl_grid(n >> 2)), dim3(kFlT), 0, st, gout, gdata, n, count);
  else
    hipLaunchKernelGGL(bbox_norm_bwd_kernel<false>, dim3(fl_grid(n)), dim3(kFlT), 0, st, gout, gdata, n, count);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
