// Error reporting, ABI version and tuning knobs of libsimpledet_ops_hip.so.
#include "common.h"
#include <stdarg.h>
#include "../../include/simpledet_ops.h"
#include <atomic>
#include <string.h>
#include <hip/hip_fp16.h>

namespace sd {

char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

namespace {
// the rows of SD_KNOBS (common.h), each with the value in effect, which starts at the row's default
struct KnobRow {
  const char* key;
  int lo, hi;
  std::atomic<int> value;
};
#define SD_KNOB_ROW(id, dflt, lo, hi, what) {#id, lo, hi, {dflt}},
KnobRow g_knobs[] = {SD_KNOBS(SD_KNOB_ROW)};
#undef SD_KNOB_ROW

KnobRow* find_knob(const char* key) {
  for (auto& k : g_knobs)
    if (!strcmp(k.key, key)) return &k;
  return nullptr;
}
}  // namespace

int tuning(Knob knob) {
  const KnobRow& k = g_knobs[(int)knob];
  const int v = k.value.load(std::memory_order_relaxed);
  return v < k.lo ? k.lo : (v > k.hi ? k.hi : v);
}

}  // namespace sd

namespace sd {
// The per-call counters of the selection operators (digit and bin histograms, candidate counts, list lengths) are
// zeroed by a kernel rather than hipMemsetAsync: they must be zero in every replay of a captured graph as well (a
// memset node was not repeated on replays here; stale counts let a finishing kernel read candidate slots its call
// never wrote).  n < 2^31 * 1.01: the grid stays under 2^24 blocks.
__global__ __launch_bounds__(256) void zero_counters_kernel(int* p, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}
void zero_counters(int* p, long n, hipStream_t stream) {
  hipLaunchKernelGGL(zero_counters_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, n);
}

// HBM streaming copy: the measured-peak companion of the 8 TB/s spec figure and the known-byte
// calibration stream for rocprofv3's FETCH_SIZE / WRITE_SIZE (MI355X_MICROARCH.md, HBM).
template <typename T>
__global__ __launch_bounds__(256) void hbm_stream_copy(const T* __restrict__ src,
                                                       T* __restrict__ dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = src[i];
}
}  // namespace sd

extern "C" int sd_hbm_stream_copy(const void* src, void* dst, size_t bytes, int width_bytes,
                                  void* stream) {
  SD_REQUIRE(src && dst, "null buffer");
  SD_REQUIRE(width_bytes == 4 || width_bytes == 8 || width_bytes == 16, "width must be 4, 8, 16");
  SD_REQUIRE(bytes % width_bytes == 0, "bytes must be a multiple of the access width");
  hipStream_t st = (hipStream_t)stream;
  const size_t n = bytes / width_bytes;
  const int grid = sd::kNumCU * 8;
  if (width_bytes == 16)
    sd::hbm_stream_copy<float4><<<grid, 256, 0, st>>>((const float4*)src, (float4*)dst, n);
  else if (width_bytes == 8)
    sd::hbm_stream_copy<float2><<<grid, 256, 0, st>>>((const float2*)src, (float2*)dst, n);
  else
    sd::hbm_stream_copy<float><<<grid, 256, 0, st>>>((const float*)src, (float*)dst, n);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

namespace sd {
// fp16 <-> fp32 streaming casts: the op-boundary casts of the fp16 RoIAlign backward (the backward
// kernel accumulates and writes fp32; its fp16 form wraps it in these two passes)
__global__ __launch_bounds__(256) void cast_h2f_kernel(const __half* __restrict__ src, float* __restrict__ dst, size_t n) {
  size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  const size_t stride = (size_t)gridDim.x * blockDim.x * 8;
  for (; i + 8 <= n; i += stride) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + i);
    const __half2* h = reinterpret_cast<const __half2*>(&v);
    const float2 a = __half22float2(h[0]), b = __half22float2(h[1]), c = __half22float2(h[2]), d = __half22float2(h[3]);
    reinterpret_cast<float4*>(dst + i)[0] = make_float4(a.x, a.y, b.x, b.y);
    reinterpret_cast<float4*>(dst + i)[1] = make_float4(c.x, c.y, d.x, d.y);
  }
  if (i < n && i + 8 > n)
    for (size_t j = i; j < n; ++j) dst[j] = __half2float(src[j]);
}
__global__ __launch_bounds__(256) void cast_f2h_kernel(const float* __restrict__ src, __half* __restrict__ dst, size_t n, int add) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    dst[i] = __float2half(add ? __half2float(dst[i]) + src[i] : src[i]);
}
}  // namespace sd

extern "C" int sd_cast_f16_to_f32(const void* src, float* dst, size_t n, void* stream) {
  if (n == 0) return SD_OK;
  SD_REQUIRE(src && dst, "null buffer");
  SD_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "buffers must be 16-byte aligned");
  sd::cast_h2f_kernel<<<sd::kNumCU * 8, 256, 0, (hipStream_t)stream>>>((const __half*)src, dst, n);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_cast_f32_to_f16(const float* src, void* dst, size_t n, int req, void* stream) {
  if (n == 0 || req == SD_REQ_NULL) return SD_OK;
  SD_REQUIRE(src && dst, "null buffer");
  SD_REQUIRE(req == SD_REQ_WRITE || req == SD_REQ_ADD, "req must be write or add");
  sd::cast_f2h_kernel<<<sd::kNumCU * 8, 256, 0, (hipStream_t)stream>>>(src, (__half*)dst, n, req == SD_REQ_ADD);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_stream_synchronize(void* stream) {
  SD_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return SD_OK;
}

namespace sd {
// the kernels the last RoIAlign entry point of this thread launched, for measurement tools
static thread_local char g_dispatch[256] = {0};
void note_dispatch(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_dispatch, sizeof(g_dispatch), fmt, ap);
  va_end(ap);
}
}  // namespace sd

extern "C" const char* sd_last_error(void) { return sd::err_buf(); }
extern "C" const char* sd_last_dispatch(void) { return sd::g_dispatch; }
extern "C" int sd_abi_version(void) { return SD_ABI_VERSION; }

extern "C" int sd_set_tuning(const char* key, int value) {
  if (!key) return sd::fail(SD_ERR_INVALID_ARG, "null tuning key");
  sd::KnobRow* k = sd::find_knob(key);
  if (!k) return sd::fail(SD_ERR_INVALID_ARG, "unknown tuning key '%s'", key);
  k->value.store(value, std::memory_order_relaxed);
  return SD_OK;
}

extern "C" int sd_get_tuning(const char* key, int* value) {
  if (!key || !value) return sd::fail(SD_ERR_INVALID_ARG, "null argument");
  const sd::KnobRow* k = sd::find_knob(key);
  if (!k) return sd::fail(SD_ERR_INVALID_ARG, "unknown tuning key '%s'", key);
  *value = k->value.load(std::memory_order_relaxed);
  return SD_OK;
}

extern "C" const char* sd_tuning_key(int index) {
  return index >= 0 && index < (int)sd::Knob::kCount ? sd::g_knobs[index].key : nullptr;
}
