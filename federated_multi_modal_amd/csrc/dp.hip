// DP-FedAvg (McMahan, Ramage, Talwar, Zhang: "Learning Differentially Private Recurrent Language Models", ICLR 2018;
// Geyer, Klein, Nabi 2017) over the flat trainable buffers: the L2 norm of a client's update w_k - w_global with the
// clip scale it implies, and the Gaussian noise added to the summed bucket.  The clipped pack itself stands beside
// pack_kernel in optim.hip; the contract of all three is in include/mapfed.h.
//
// Every fp32 operation below is rounded on its own (no fused multiply-add), no float atomics, and the
// transcendental functions are the correctly-specified library ones (logf, sqrtf, sinf, cosf), not the hardware
// approximations.
#include "mf_common.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace {

constexpr int CHUNK = 8192;  // elements per block of the first launch: 32 per thread

inline unsigned nblk(int64_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }
inline int64_t nchunks(int64_t n) { return (n + CHUNK - 1) / CHUNK; }

MF_DEV float sq_diff(float p, float g) {
  const float d = p - g;
  return d * d;
}

// sum over [start, end) of (float(p_i) - float(g_i))^2 as this thread's share: 16-byte loads over the middle that is
// 16-byte aligned in both buffers, element loads for the ragged ends (and throughout when p and g are not aligned
// alike)
template <typename T>
MF_DEV float chunk_sumsq(const T* __restrict__ p, const T* __restrict__ g, int64_t start, int64_t end) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec __attribute__((ext_vector_type(V)));
  int64_t a = start + (int64_t)(((16 - ((uintptr_t)(p + start) & 15)) & 15) / sizeof(T));
  if (a > end || ((uintptr_t)(g + a) & 15) != 0) a = end;
  const int64_t nv = (end - a) / V, b = a + nv * V;
  float s = 0.f;
  for (int64_t i = start + threadIdx.x; i < a; i += blockDim.x) s += sq_diff((float)p[i], (float)g[i]);
  const vec* pv = (const vec*)(p + a);
  const vec* gv = (const vec*)(g + a);
  for (int64_t i = threadIdx.x; i < nv; i += blockDim.x) {
    const vec x = pv[i], y = gv[i];
#pragma unroll
    for (int e = 0; e < V; ++e) s += sq_diff((float)x[e], (float)y[e]);
  }
  for (int64_t i = b + threadIdx.x; i < end; i += blockDim.x) s += sq_diff((float)p[i], (float)g[i]);
  return s;
}

// blocks [0, nc16) take the fp16 buffers' chunks, the rest the fp32 buffers'; part[block] = the chunk's fp32 sum
__global__ __launch_bounds__(256) void dp_sumsq_kernel(const f16* __restrict__ p16, const f16* __restrict__ g16,
                                                       int64_t n16, const float* __restrict__ p32,
                                                       const float* __restrict__ g32, int64_t n32, unsigned nc16,
                                                       float* __restrict__ part) {
  float s;
  if (blockIdx.x < nc16) {
    const int64_t start = (int64_t)blockIdx.x * CHUNK;
    s = chunk_sumsq<f16>(p16, g16, start, min(n16, start + CHUNK));
  } else {
    const int64_t start = (int64_t)(blockIdx.x - nc16) * CHUNK;
    s = chunk_sumsq<float>(p32, g32, start, min(n32, start + CHUNK));
  }
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One block: the partial sums in chunk order in fp64 (thread t sums a contiguous run of chunks, thread 0 the 256 runs
// in order), then out = {norm, scale, clipped}: scale = clip / norm when norm > clip, else exactly 1 (a NaN norm
// compares false: the validity flag deals with that client)
__global__ __launch_bounds__(256) void dp_scale_kernel(const float* __restrict__ part, int64_t nparts, float clip,
                                                       float* __restrict__ out) {
  __shared__ double run[256];
  const int64_t per = (nparts + 255) / 256;
  const int64_t lo = min(nparts, (int64_t)threadIdx.x * per), hi = min(nparts, lo + per);
  double s = 0.0;
  for (int64_t c = lo; c < hi; ++c) s += (double)part[c];
  run[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int t = 0; t < 256; ++t) tot += run[t];
    const float norm = (float)sqrt(tot);
    const bool clipped = norm > clip;
    out[0] = norm;
    out[1] = clipped ? clip / norm : 1.f;
    out[2] = clipped ? 1.f : 0.f;
  }
}

// 23 random bits to an odd multiple of 2^-24: exact in fp32, in (0, 1)
MF_DEV float unit_open(uint32_t x) { return (float)(((x >> 9) << 1) | 1u) * 0x1p-24f; }

MF_DEV void box_muller(uint32_t xa, uint32_t xb, float& even, float& odd) {
  const float r = sqrtf(-2.f * logf(unit_open(xa)));
  const float theta = 6.2831855f * unit_open(xb);
  even = r * cosf(theta);
  odd = r * sinf(theta);
}

// One thread per Philox counter q = q0 + t, the four global coordinates 4q .. 4q + 3 = buf[4q - offset ...].  The
// four normals are formed first; only the access differs: one 16-byte load and store when the counter lies wholly
// inside [0, n) and `vec` (its address is 16-byte aligned: the same answer for every counter), element accesses
// otherwise, so a call's first and last counters may be partial
__global__ __launch_bounds__(256) void dp_noise_kernel(float* __restrict__ buf, int64_t n, uint64_t offset,
                                                       uint64_t q0, int64_t nq, uint32_t k0, uint32_t k1,
                                                       uint32_t round, float std, int vec) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nq) return;
  const uint64_t q = q0 + (uint64_t)t;
  uint32_t x[4];
  philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), round, 0u, k0, k1, x);
  float z[4];
  box_muller(x[0], x[1], z[0], z[1]);
  box_muller(x[2], x[3], z[2], z[3]);
  const int64_t j0 = (int64_t)(4 * q - offset);  // -3 .. n - 1
  if (vec && j0 >= 0 && j0 + 4 <= n) {
    f32x4 v = *(const f32x4*)(buf + j0);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const float add = std * z[l];
      v[l] = v[l] + add;
    }
    *(f32x4*)(buf + j0) = v;
  } else {
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int64_t j = j0 + l;
      if (j >= 0 && j < n) {
        const float add = std * z[l];
        buf[j] = buf[j] + add;
      }
    }
  }
}

}  // namespace

// floats of workspace mf_dp_update_scale needs: one partial sum per chunk of either buffer (at least one)
extern "C" int64_t mf_dp_update_ws_floats(int64_t n16, int64_t n32) {
  if (n16 < 0 || n32 < 0) return -1;
  const int64_t nc = nchunks(n16) + nchunks(n32);
  return nc > 0 ? nc : 1;
}

extern "C" int mf_dp_update_scale(const void* p16, const void* g16, int64_t n16, const float* p32, const float* g32,
                                  int64_t n32, float clip, float* ws, float* out, void* stream) {
  if (n16 < 0 || n32 < 0) return mf_set_error("mf_dp_update_scale: negative size", -1);
  if (!(clip > 0.f) || __builtin_isnan(clip)) return mf_set_error("mf_dp_update_scale: clip not > 0", -1);
  if (!ws || !out) return mf_set_error("mf_dp_update_scale: null workspace or out", -1);
  if ((n16 > 0 && (!p16 || !g16)) || (n32 > 0 && (!p32 || !g32)))
    return mf_set_error("mf_dp_update_scale: null weights or global copy", -1);
  const int64_t nc16 = nchunks(n16), nc32 = nchunks(n32);
  if (nc16 + nc32 > 0x7fffffff) return mf_set_error("mf_dp_update_scale: too many chunks for one launch", -1);
  hipStream_t st = (hipStream_t)stream;
  if (nc16 + nc32 > 0) {
    dp_sumsq_kernel<<<(unsigned)(nc16 + nc32), 256, 0, st>>>((const f16*)p16, (const f16*)g16, n16, p32, g32, n32,
                                                             (unsigned)nc16, ws);
    MF_CHECK_LAUNCH();
  }
  dp_scale_kernel<<<1, 256, 0, st>>>(ws, nc16 + nc32, clip, out);
  MF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mf_dp_add_noise(float* buf, int64_t n, int64_t offset, uint64_t seed, uint32_t round, float std,
                               void* stream) {
  if (n < 0 || offset < 0) return mf_set_error("mf_dp_add_noise: negative n or offset", -1);
  if (offset > INT64_MAX - n) return mf_set_error("mf_dp_add_noise: offset + n overflows", -1);
  if (!(std >= 0.f) || __builtin_isinf(std)) return mf_set_error("mf_dp_add_noise: std not finite and >= 0", -1);
  if (n == 0 || std == 0.f) return 0;  // x + 0 * z would still turn a -0 into +0
  if (!buf) return mf_set_error("mf_dp_add_noise: null buffer", -1);
  if ((uintptr_t)buf % 4 != 0) return mf_set_error("mf_dp_add_noise: buffer not 4-byte aligned", -1);
  const uint64_t q0 = (uint64_t)offset >> 2, q1 = (uint64_t)(offset + n - 1) >> 2;
  const int64_t nq = (int64_t)(q1 - q0) + 1;
  if (nq > (int64_t)0x7fffffff * 256) return mf_set_error("mf_dp_add_noise: n too large for one launch", -1);
  // the address of counter q0's first coordinate (it may lie up to 3 floats before buf): 16-byte aligned or not,
  // and every later counter is a multiple of 16 bytes further on
  const uintptr_t first = (uintptr_t)buf + 4 * (4 * q0 - (uint64_t)offset);
  dp_noise_kernel<<<nblk(nq), 256, 0, (hipStream_t)stream>>>(buf, n, (uint64_t)offset, q0, nq, (uint32_t)seed,
                                                             (uint32_t)(seed >> 32), round, std, first % 16 == 0);
  MF_CHECK_LAUNCH();
  return 0;
}
