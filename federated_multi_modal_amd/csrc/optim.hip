// Optimizer step and federated averaging over the flat trainable buffers.
//
// The trainable tensors (trainers/maple.py:447-479) live in two flat device buffers, one fp16 and
// one fp32, each tensor a contiguous segment; grads and SGD momentum mirror them.  That turns
//   torch.nn.utils.clip_grad_norm_(params, 1.0)      (trainers/maple.py:592-596)
//   Dassl SGD(momentum 0.9, wd 5e-4).step()           (trainers/maple.py:598)
//   safe_average_weights / check_weights_valid        (trainers/maple_fed.py:309-325)
// into a handful of streaming kernels with no host synchronisation: the clip coefficient stays on
// the device and the SGD kernel reads it.
//
// Rounding points follow torch: per-tensor norms in the grad's dtype (fp16 norm for fp16 grads),
// total norm in fp32, coef = clamp(1/(total+1e-6), max 1); g = T(g*coef); d_p = T(g + wd*p);
// buf = d_p (first step) or T(T(buf*mom) + d_p); p = T(p - lr*buf).
#include <cstdio>
#include <type_traits>
#include <utility>

#include "mf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CHUNK = 8192;

typedef float f32x8 __attribute__((ext_vector_type(8)));
// 8 consecutive elements of a flat buffer: one 16-byte (fp16) or two 16-byte (fp32) accesses
template <typename T>
using vec8 = typename std::conditional<std::is_same<T, f16>::value, f16x8, f32x8>::type;

inline unsigned nblk(int64_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }
inline bool aligned(const void* p, uintptr_t bytes) { return (uintptr_t)p % bytes == 0; }

struct Chunk {
  int seg;
  int is16;
  int64_t start, end;  // element range inside the segment's flat buffer
};

__global__ void sumsq_chunks_kernel(const f16* __restrict__ g16, const float* __restrict__ g32,
                                    const Chunk* __restrict__ chunks, float* __restrict__ part) {
  const Chunk c = chunks[blockIdx.x];
  float s = 0.f;
  // 16-byte loads over the chunk's 16-byte-aligned middle (the flat buffers are 256-B aligned), element
  // loads for the ragged head and tail
  if (c.is16) {
    const int64_t a = min(c.end, (c.start + 7) & ~(int64_t)7), b = max(a, c.end & ~(int64_t)7);
    for (int64_t i = c.start + threadIdx.x; i < a; i += blockDim.x) {
      float v = (float)g16[i];
      s += v * v;
    }
    for (int64_t i = a / 8 + threadIdx.x; i < b / 8; i += blockDim.x) {
      const f16x8 v = ((const f16x8*)g16)[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) s += (float)v[e] * (float)v[e];
    }
    for (int64_t i = b + threadIdx.x; i < c.end; i += blockDim.x) {
      float v = (float)g16[i];
      s += v * v;
    }
  } else {
    const int64_t a = min(c.end, (c.start + 3) & ~(int64_t)3), b = max(a, c.end & ~(int64_t)3);
    for (int64_t i = c.start + threadIdx.x; i < a; i += blockDim.x) {
      float v = g32[i];
      s += v * v;
    }
    for (int64_t i = a / 4 + threadIdx.x; i < b / 4; i += blockDim.x) {
      const f32x4 v = ((const f32x4*)g32)[i];
      s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    for (int64_t i = b + threadIdx.x; i < c.end; i += blockDim.x) {
      float v = g32[i];
      s += v * v;
    }
  }
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// One block of 1024 threads: per-segment norms from the per-chunk partial sums (the chunks of a
// segment are consecutive), total norm, clip coefficient.  The chunk list is walked in tiles of 1024
// with a segmented inclusive scan (Hillis-Steele in LDS, fixed order -> deterministic); the last
// chunk of each segment yields that segment's sum of squares (plus the carry of a segment that
// started in an earlier tile).  torch.nn.utils.clip_grad_norm_: per-tensor norms in the grad's dtype
// (fp16 tensors round their norm to fp16), total = ||(norm_t)_t||_2 in fp32,
// coef = clamp(max_norm / (total + 1e-6), max 1).
// out[0] = total norm, out[1] = clip coef, out[2] = 1 if total is finite else 0
__global__ __launch_bounds__(1024) void clip_coef_kernel(const float* __restrict__ part,
                                                         const Chunk* __restrict__ chunks, int nchunks,
                                                         float max_norm, float* __restrict__ out,
                                                         float* __restrict__ hyper = nullptr,
                                                         const float* __restrict__ halt_src = nullptr,
                                                         const int* __restrict__ halt_src2 = nullptr) {
  __shared__ float sv[1024];
  __shared__ int sseg[1024];
  __shared__ float red[16];
  __shared__ float carry_val;
  __shared__ int carry_seg;
  const int t = threadIdx.x;
  if (t == 0) {
    carry_val = 0.f;
    carry_seg = -1;
  }
  float acc = 0.f;
  for (int base = 0; base < nchunks; base += 1024) {
    const int c = base + t;
    const int seg = c < nchunks ? chunks[c].seg : -1;
    float v = c < nchunks ? part[c] : 0.f;
    sseg[t] = seg;
    sv[t] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      float add = 0.f;
      if (t >= off && sseg[t - off] == seg) add = sv[t - off];
      __syncthreads();
      v += add;
      sv[t] = v;
      __syncthreads();
    }
    const bool last = c < nchunks && (c == nchunks - 1 || chunks[c + 1].seg != seg);
    if (last) {
      float ss = v;
      if (seg == carry_seg && sseg[0] == seg) ss += carry_val;  // segment began in an earlier tile
      float nrm = sqrtf(ss);
      if (chunks[c].is16) nrm = r16(nrm);
      acc += nrm * nrm;
    }
    __syncthreads();
    if (t == 1023) {
      const float prev = (seg == carry_seg && sseg[0] == seg) ? carry_val : 0.f;
      carry_val = v + prev;
      carry_seg = seg;
    }
    __syncthreads();
  }
  acc = wave_sum(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    float tot = 0.f;
    for (int i = 0; i < 16; ++i) tot += red[i];
    const float total = sqrtf(tot);
    float coef = max_norm / (total + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;
    out[0] = total;
    out[1] = coef;
    out[2] = isfinite(total) ? 1.f : 0.f;
    // the step's halt latch (torch.maximum(hyper[4], loss non-finite flag)) for the SGD launch that follows
    if (hyper) {
      const float h = fmaxf(hyper[4], halt_src[0]);
      hyper[4] = halt_src2 ? fmaxf(h, (float)halt_src2[0]) : h;
    }
  }
}

// hyper = {lr, momentum, weight_decay, first_step (1.0 = momentum buffer not yet created), halt}: read from
// device memory so a captured step replays with the current schedule value.  halt != 0 (a non-finite loss
// earlier in the epoch or in this step) leaves parameters, gradients and momentum untouched: the reference
// raises at the first non-finite loss before its backward (trainers/maple.py:375-376), so no update follows.
//
// FedProx (Li et al., "Federated Optimization in Heterogeneous Networks", MLSys 2020): the local objective gains
// (mu/2) * ||w - w_global||^2, whose gradient mu * (w - w_global) joins the clipped gradient in the optimizer, as
// weight decay does.  hyper = {lr, momentum, weight_decay, first_step, halt, mu}.  Every line rounded to T, as
// torch ops on T tensors round: gc = T(g*coef) (stored back: the stored gradient stays the clipped model
// gradient); d = T(p - pglob); gp = T(gc + mu*d); d_p = T(gp + wd*p); momentum and parameter update as the plain
// step.  pglob is read only and must not overlap p, g or buf.
//
// FedDyn (Acar et al., "Federated Learning Based on Dynamic Regularization", ICLR 2021): the local objective gains
// -<lam, w> + (alpha/2) * ||w - w_global||^2, so the proximal line (alpha in mu's slot, hyper[5]) is followed by
// gl = T(gp - lam): lam is the client's fp32 linear correction (read only, n elements in the buffer's order, whatever
// T is), the difference one fp32 subtraction rounded to T.
//
// The plain, the proximal and the dynamic step are the three instantiations of one element function, one scalar
// kernel, one 8-wide body and one fused kernel, so each rounding is written once.  SGD_PLAIN reads neither pglob
// (null) nor hyper[5] (the plain callers' hyper has 5 floats); lam (null otherwise) is read by SGD_DYN alone.
enum { SGD_PLAIN = 0, SGD_PROX = 1, SGD_DYN = 2 };

// fp32 difference of a and b, materialised as fp32 before any fp16 rounding of it, as mul32 materialises a product:
// fp16(a - b) with an fp32 b must not become one mixed-precision operation that rounds the exact difference once
MF_DEV float sub32(float a, float b) {
  float d = a - b;
  asm volatile("" : "+v"(d));
  return d;
}

template <typename T, int MODE>
MF_DEV void sgd_elem(float pe, float ge, float be, float qe, float le, float coef, float lr, float momentum, float wd,
                     float mu, bool first, float& p_out, float& g_out, float& b_out) {
  const float gc = (float)(T)mul32(ge, coef);
  g_out = gc;
  float gp = gc;
  if constexpr (MODE != SGD_PLAIN) {
    const float d = (float)(T)(pe - qe);
    gp = (float)(T)(gc + mul32(mu, d));
  }
  if constexpr (MODE == SGD_DYN) gp = (float)(T)sub32(gp, le);
  const float dp = (float)(T)(gp + wd * pe);
  float b;
  if (first)
    b = dp;
  else
    b = (float)(T)((float)(T)mul32(be, momentum) + dp);
  b_out = b;
  p_out = (float)(T)(pe + (-lr) * b);
}

template <typename T, int MODE>
__global__ void sgd_kernel(T* __restrict__ p, T* __restrict__ g, T* __restrict__ buf, const T* __restrict__ pglob,
                           const float* __restrict__ lam, int64_t n, const float* __restrict__ coef_ptr,
                           const float* __restrict__ hyper) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || hyper[4] != 0.f) return;
  const bool first = hyper[3] != 0.f;
  float qe = 0.f, le = 0.f, po, go, bo;
  if constexpr (MODE != SGD_PLAIN) qe = (float)pglob[i];
  if constexpr (MODE == SGD_DYN) le = lam[i];
  sgd_elem<T, MODE>((float)p[i], (float)g[i], first ? 0.f : (float)buf[i], qe, le, coef_ptr[1], hyper[0], hyper[1],
                    hyper[2], MODE != SGD_PLAIN ? hyper[5] : 0.f, first, po, go, bo);
  g[i] = (T)go;
  buf[i] = (T)bo;
  p[i] = (T)po;
}

// sgd_kernel on 8 consecutive elements per thread (16-byte fp16 / 2 x 16-byte fp32 accesses, the proximal step one
// more read of the global copy, the dynamic one 32 bytes of lam besides), the same per-element arithmetic; n % 8 == 0
// and 32-byte aligned buffers
template <typename T, int MODE>
MF_DEV void sgd8_body(T* __restrict__ p, T* __restrict__ g, T* __restrict__ buf, const T* __restrict__ pglob,
                      const float* __restrict__ lam, int64_t n8, int64_t i, const float* __restrict__ coef_ptr,
                      const float* __restrict__ hyper) {
  using V = vec8<T>;
  if (i >= n8 || hyper[4] != 0.f) return;
  const float coef = coef_ptr[1];
  const float lr = hyper[0], momentum = hyper[1], wd = hyper[2], mu = MODE != SGD_PLAIN ? hyper[5] : 0.f;
  const bool first = hyper[3] != 0.f;
  V pv = ((V*)p)[i], gv = ((V*)g)[i], bv = first ? V{} : ((V*)buf)[i], qv{};
  f32x8 lv{};
  if constexpr (MODE != SGD_PLAIN) qv = ((const V*)pglob)[i];
  if constexpr (MODE == SGD_DYN) lv = ((const f32x8*)lam)[i];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float po, go, bo;
    sgd_elem<T, MODE>((float)pv[e], (float)gv[e], (float)bv[e], (float)qv[e], lv[e], coef, lr, momentum, wd, mu, first,
                      po, go, bo);
    gv[e] = (T)go;
    bv[e] = (T)bo;
    pv[e] = (T)po;
  }
  ((V*)g)[i] = gv;
  ((V*)buf)[i] = bv;
  ((V*)p)[i] = pv;
}

template <typename T, int MODE>
__global__ void sgd8_kernel(T* __restrict__ p, T* __restrict__ g, T* __restrict__ buf, const T* __restrict__ pglob,
                            const float* __restrict__ lam, int64_t n8, const float* __restrict__ coef_ptr,
                            const float* __restrict__ hyper) {
  sgd8_body<T, MODE>(p, g, buf, pglob, lam, n8, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, coef_ptr, hyper);
}

// both flat buffers' SGD in one launch: blocks [0, nb16) update the fp16 trainables, the rest the fp32 ones; lam16 /
// lam32 are lam and lam + n16
template <int MODE>
__global__ void sgd8_both_kernel(f16* __restrict__ p16, f16* __restrict__ g16, f16* __restrict__ b16,
                                 const f16* __restrict__ q16, const float* __restrict__ lam16, int64_t n16_8,
                                 float* __restrict__ p32, float* __restrict__ g32, float* __restrict__ b32,
                                 const float* __restrict__ q32, const float* __restrict__ lam32, int64_t n32_8,
                                 unsigned nb16, const float* __restrict__ coef_ptr, const float* __restrict__ hyper) {
  if (blockIdx.x < nb16)
    sgd8_body<f16, MODE>(p16, g16, b16, q16, lam16, n16_8, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, coef_ptr,
                         hyper);
  else
    sgd8_body<float, MODE>(p32, g32, b32, q32, lam32, n32_8, (int64_t)(blockIdx.x - nb16) * blockDim.x + threadIdx.x,
                           coef_ptr, hyper);
}

// A client's bucket, plain: bucket[0:n16] = float(p16), bucket[n16:n] = p32 (n = n16 + n32), bucket[n] = 1, this
// client's vote in the valid-client count.  Weighted, FedAvg as McMahan et al. define it ("Communication-Efficient
// Learning of Deep Networks from Decentralized Data", AISTATS 2017): w_global = sum_k n_k w_k / sum_k n_k.  The
// client's weight travels in its bucket: bucket[0:n] = w * float(p) (the fp32 product is formed and stored here; the
// sum is formed by reduce_ordered_kernel, so no fused multiply-add spans the two), bucket[n] = w, bucket[n+1] = 1
// (its vote).  An invalid client (maple_fed.py:272-277) writes zeros everywhere -- or, ABSENT (the robust
// aggregation's bucket: the weighted layout at w = 1, and 1.f * x is x), the quiet NaN reduce_trimmed_kernel reads as
// "this client is absent", since a zero would take part in a median.
template <bool WEIGHTED>
constexpr int TAIL = WEIGHTED ? 2 : 1;

// CLIP (DP-FedAvg, McMahan et al., ICLR 2018): the client's update x - g is scaled by s = *scale (mf_dp_update_scale's
// out[1], read on the device) before it is packed, and the bucket still holds weights: y = g + s * (x - g), three
// separately rounded fp32 operations.  s >= 1 selects x itself, so a client inside the bound packs the bits the
// other instantiations pack.  g16 / g32 / scale are read by CLIP only (null otherwise).
template <bool WEIGHTED, bool ABSENT = false, bool CLIP = false>
__global__ void pack_kernel(const f16* __restrict__ p16, int64_t n16, const float* __restrict__ p32, int64_t n32,
                            const int* __restrict__ invalid, float* __restrict__ bucket, float w,
                            const f16* __restrict__ g16 = nullptr, const float* __restrict__ g32 = nullptr,
                            const float* __restrict__ scale = nullptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = n16 + n32;
  const bool bad = invalid && invalid[0] != 0;
  const float none = ABSENT ? __int_as_float(0x7fc00000) : 0.f;
  float s = 1.f;
  if constexpr (CLIP) s = scale[0];
  const auto weigh = [&](float x, float g) {
    if constexpr (CLIP) {
      const float d = x - g;
      const float sd = s * d;
      const float y = g + sd;
      x = s >= 1.f ? x : y;
    }
    if constexpr (WEIGHTED)
      return w * x;
    else
      return x;
  };
  if (i < n16)
    bucket[i] = bad ? none : weigh((float)p16[i], CLIP ? (float)g16[i] : 0.f);
  else if (i < n)
    bucket[i] = bad ? none : weigh(p32[i - n16], CLIP ? g32[i - n16] : 0.f);
  else if (i == n)
    bucket[i] = bad ? none : (WEIGHTED ? w : 1.f);
  else if (WEIGHTED && i == n + 1)
    bucket[i] = bad ? none : 1.f;
}

// fp16 `val` to element i of [fp16 trainables | fp32 trainables] and of the global copy (g16 / g32 may be null)
MF_DEV void deliver(f16 val, int64_t i, f16* __restrict__ p16, int64_t n16, float* __restrict__ p32,
                    f16* __restrict__ g16, float* __restrict__ g32) {
  if (i < n16) {
    p16[i] = val;
    if (g16) g16[i] = val;
  } else {
    p32[i - n16] = (float)val;
    if (g32) g32[i - n16] = (float)val;
  }
}
// ... and the global copy's element i back into the trainables
MF_DEV void restore(int64_t i, f16* __restrict__ p16, int64_t n16, float* __restrict__ p32,
                    const f16* __restrict__ g16, const float* __restrict__ g32) {
  if (i < n16) {
    if (g16) p16[i] = g16[i];
  } else {
    if (g32) p32[i - n16] = g32[i - n16];
  }
}
// the same for 8 consecutive elements of one buffer: fp16(x[e]), one 16-byte fp16 / 32-byte fp32 store each
template <typename T>
MF_DEV void deliver8(const f32x8& x, T* __restrict__ p, T* __restrict__ g, int64_t i) {
  vec8<T> out;
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = (T)(f16)x[e];
  ((vec8<T>*)p)[i] = out;
  ((vec8<T>*)g)[i] = out;
}

// mean = sum / d with d = bucket[n] read on the device (no host sync): the valid-client count of the plain layout,
// the summed weights of the weighted one; value = fp16(mean); p16 = value, p32 = float(value)   (the `.half()` of
// trainers/maple_fed.py:314 followed by load_state_dict into each parameter's dtype), and the value is kept as the
// new global copy (g16/g32).  No votes (bucket[n + TAIL - 1] == 0) -> every client failed: the round is skipped and
// every client goes back to the previous global weights (trainers/maple_fed.py:288-290 + the next round's broadcast).
template <bool WEIGHTED>
__global__ void unpack_kernel(const float* __restrict__ bucket, f16* __restrict__ p16, int64_t n16,
                              float* __restrict__ p32, int64_t n32, f16* __restrict__ g16, float* __restrict__ g32) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = n16 + n32;
  if (i >= n) return;
  const float d = bucket[n], votes = bucket[n + TAIL<WEIGHTED> - 1];
  if (votes == 0.f)
    restore(i, p16, n16, p32, g16, g32);
  else
    deliver((f16)(bucket[i] / d), i, p16, n16, p32, g16, g32);
}

// FedOpt server optimizers: FedAvgM (Hsu, Qi, Brown: "Measuring the Effects of Non-Identical Data Distribution for
// Federated Visual Classification", 2019) and FedAdagrad / FedAdam / FedYogi (Reddi et al., "Adaptive Federated
// Optimization", ICLR 2021, Algorithm 2, no bias correction).  The step replaces unpack_kernel on the summed bucket:
// the mean is the pseudo-gradient's target, the server keeps an fp32 master copy x of the trainables (a step
// eta * m / (sqrt(v) + tau) is lost in an fp16 weight) with its moments m and v, and the clients receive fp16(x),
// what a `.half()` state dict would hold.  Per element, every binary operation rounded to fp32 once, no fused
// multiply-add (the file's contract(off)):
//   mean = sum / d;  delta = mean - x
//   fedavgm:    m = b1*m + delta;                               upd = m
//   adaptive:   m = b1*m + (1-b1)*delta;  s = delta*delta
//     fedadagrad: v = v + s
//     fedadam:    v = b2*v + (1-b2)*s
//     fedyogi:    v = v - ((1-b2)*s) * sign(v - s)   (sign(0) = 0)
//                                                               upd = m / (sqrtf(v) + tau)
//   x = x + eta*upd
enum { FEDOPT_AVGM = 1, FEDOPT_ADAGRAD = 2, FEDOPT_ADAM = 3, FEDOPT_YOGI = 4 };

struct FedOptHyper {
  int opt;
  float b1, b2, tau, eta;
};

MF_DEV void fedopt_elem(const FedOptHyper& h, float omb1, float omb2, float sum, float d, float& x, float& m,
                        float& v) {
  const float mean = sum / d;
  const float delta = mean - x;
  float upd;
  if (h.opt == FEDOPT_AVGM) {
    m = h.b1 * m + delta;
    upd = m;
  } else {
    m = h.b1 * m + omb1 * delta;
    const float s = delta * delta;
    if (h.opt == FEDOPT_ADAGRAD) {
      v = v + s;
    } else if (h.opt == FEDOPT_ADAM) {
      v = h.b2 * v + omb2 * s;
    } else {
      const float t = v - s;
      const float sg = t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f);
      v = v - (omb2 * s) * sg;
    }
    upd = m / (sqrtf(v) + h.tau);
  }
  x = x + h.eta * upd;
}

// one element per thread over [fp16 trainables | fp32 trainables]; d = bucket[n] (the vote count of the plain
// layout, the summed weights of the weighted one), votes = bucket[n + weighted].  No votes: the client goes back to
// the global copy and the server state keeps its bits.
__global__ void fedopt_step_kernel(const float* __restrict__ bucket, int weighted, FedOptHyper h,
                                   float* __restrict__ x, float* __restrict__ m, float* __restrict__ v,
                                   f16* __restrict__ p16, int64_t n16, float* __restrict__ p32, int64_t n32,
                                   f16* __restrict__ g16, float* __restrict__ g32) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = n16 + n32;
  if (i >= n) return;
  const float d = bucket[n], votes = bucket[n + weighted];
  if (votes == 0.f) return restore(i, p16, n16, p32, g16, g32);
  const bool adaptive = h.opt != FEDOPT_AVGM;
  float xe = x[i], me = m[i], ve = adaptive ? v[i] : 0.f;
  fedopt_elem(h, 1.f - h.b1, 1.f - h.b2, bucket[i], d, xe, me, ve);
  x[i] = xe;
  m[i] = me;
  if (adaptive) v[i] = ve;
  deliver((f16)xe, i, p16, n16, p32, g16, g32);
}

// fedopt_step_kernel on 8 consecutive elements per thread (32-byte fp32 accesses of the bucket and the state,
// 16-byte fp16 / 32-byte fp32 stores of the weights): bucket, x, m, v already offset to this buffer's part; n % 8 == 0
// and aligned pointers (the launcher checks).  FedAvgM neither reads nor writes v.
template <typename T>
MF_DEV void fedopt8_body(const float* __restrict__ bucket, const FedOptHyper& h, float d, float votes,
                         float* __restrict__ x, float* __restrict__ m, float* __restrict__ v, T* __restrict__ p,
                         T* __restrict__ g, int64_t n8, int64_t i) {
  if (i >= n8) return;
  if (votes == 0.f) {
    ((vec8<T>*)p)[i] = ((const vec8<T>*)g)[i];
    return;
  }
  const bool adaptive = h.opt != FEDOPT_AVGM;
  const f32x8 sv = ((const f32x8*)bucket)[i];
  f32x8 xv = ((f32x8*)x)[i], mv = ((f32x8*)m)[i], vv = adaptive ? ((f32x8*)v)[i] : f32x8{};
  const float omb1 = 1.f - h.b1, omb2 = 1.f - h.b2;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float xe = xv[e], me = mv[e], ve = vv[e];
    fedopt_elem(h, omb1, omb2, sv[e], d, xe, me, ve);
    xv[e] = xe;
    mv[e] = me;
    vv[e] = ve;
  }
  ((f32x8*)x)[i] = xv;
  ((f32x8*)m)[i] = mv;
  if (adaptive) ((f32x8*)v)[i] = vv;
  deliver8<T>(xv, p, g, i);
}

// both flat buffers in one launch, split as sgd8_both_kernel splits them: blocks [0, nb16) the fp16 trainables
__global__ void fedopt8_step_kernel(const float* __restrict__ bucket, int weighted, FedOptHyper h,
                                    float* __restrict__ x, float* __restrict__ m, float* __restrict__ v,
                                    f16* __restrict__ p16, int64_t n16, float* __restrict__ p32, int64_t n32,
                                    f16* __restrict__ g16, float* __restrict__ g32, unsigned nb16) {
  const int64_t n = n16 + n32;
  const float d = bucket[n], votes = bucket[n + weighted];
  if (blockIdx.x < nb16)
    fedopt8_body<f16>(bucket, h, d, votes, x, m, v, p16, g16, n16 / 8,
                      (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  else
    fedopt8_body<float>(bucket + n16, h, d, votes, x + n16, m + n16, v ? v + n16 : v, p32, g32, n32 / 8,
                        (int64_t)(blockIdx.x - nb16) * blockDim.x + threadIdx.x);
}

// fp16(x) into another client's trainables and global copy (the rank's second and later clients)
__global__ void fedopt_deliver_kernel(const float* __restrict__ x, f16* __restrict__ p16, int64_t n16,
                                      float* __restrict__ p32, int64_t n32, f16* __restrict__ g16,
                                      float* __restrict__ g32) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n16 + n32) deliver((f16)x[i], i, p16, n16, p32, g16, g32);
}

template <typename T>
MF_DEV void deliver8_body(const float* __restrict__ x, T* __restrict__ p, T* __restrict__ g, int64_t n8, int64_t i) {
  if (i < n8) deliver8<T>(((const f32x8*)x)[i], p, g, i);
}

__global__ void fedopt8_deliver_kernel(const float* __restrict__ x, f16* __restrict__ p16, int64_t n16,
                                       float* __restrict__ p32, int64_t n32, f16* __restrict__ g16,
                                       float* __restrict__ g32, unsigned nb16) {
  if (blockIdx.x < nb16)
    deliver8_body<f16>(x, p16, g16, n16 / 8, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  else
    deliver8_body<float>(x + n16, p32, g32, n32 / 8, (int64_t)(blockIdx.x - nb16) * blockDim.x + threadIdx.x);
}

// FedDyn's round end (Acar et al., ICLR 2021, Algorithm 1) in unpack_kernel's place on the plain bucket [sum | votes].
// Per element, with w the client's local weight and q the round's starting weight (its global copy), both read before
// anything is written, every binary operation one fp32 operation (the file's contract(off)):
//   client (flag[0] == 0):  lam = lam - alpha * (w - q)             the client's gradient estimate at its optimum
//   server (STEP):          mean = sum / votes;  h = h - af * (mean - q),  af = alpha * (votes / N)
//   both:                   x = mean - h / alpha;  val = fp16(x) delivered as unpack_kernel delivers the mean
// h is the mean of the N clients' lam by construction: an absent client keeps its lam and reaches h through votes / N.
// STEP = false (the rank's second and later clients) reads the stepped h and the same bucket, so it recomputes the
// same x: no fp32 copy of x is kept.  No votes: the client goes back to its global copy, h and lam keep their bits.
struct DynRound {
  float alpha, af, votes;
  bool take;  // this client took part: its lam is updated
};

template <bool STEP>
MF_DEV DynRound dyn_round(const float* __restrict__ bucket, int64_t n, float alpha, int num_clients,
                          const int* __restrict__ flag) {
  const float votes = bucket[n];
  float af = 0.f;
  if constexpr (STEP) {
    const float frac = votes / (float)num_clients;
    af = alpha * frac;
  }
  return {alpha, af, votes, flag[0] == 0};
}

template <bool STEP>
MF_DEV float feddyn_elem(const DynRound& r, float sum, float w, float q, float& h, float& lam) {
  if (r.take) {
    const float d = w - q;
    const float ad = r.alpha * d;
    lam = lam - ad;
  }
  const float mean = sum / r.votes;
  if constexpr (STEP) {
    const float dm = mean - q;
    const float t = r.af * dm;
    h = h - t;
  }
  const float hq = h / r.alpha;
  return mean - hq;
}

// one element per thread over [fp16 trainables | fp32 trainables]
template <bool STEP>
__global__ void feddyn_kernel(const float* __restrict__ bucket, float alpha, int num_clients, float* __restrict__ h,
                              float* __restrict__ lam, const int* __restrict__ flag, f16* __restrict__ p16,
                              int64_t n16, float* __restrict__ p32, int64_t n32, f16* __restrict__ g16,
                              float* __restrict__ g32) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = n16 + n32;
  if (i >= n) return;
  const DynRound r = dyn_round<STEP>(bucket, n, alpha, num_clients, flag);
  if (r.votes == 0.f) return restore(i, p16, n16, p32, g16, g32);
  const float w = i < n16 ? (float)p16[i] : p32[i - n16], q = i < n16 ? (float)g16[i] : g32[i - n16];
  float he = h[i], le = r.take ? lam[i] : 0.f;
  const float x = feddyn_elem<STEP>(r, bucket[i], w, q, he, le);
  if (r.take) lam[i] = le;
  if constexpr (STEP) h[i] = he;
  deliver((f16)x, i, p16, n16, p32, g16, g32);
}

// feddyn_kernel on 8 consecutive elements per thread of one buffer, as fedopt8_body: bucket, h, lam already offset
// to this buffer's part; n % 8 == 0 and aligned pointers (the launcher checks)
template <typename T, bool STEP>
MF_DEV void feddyn8_body(const float* __restrict__ bucket, const DynRound& r, float* __restrict__ h,
                         float* __restrict__ lam, T* __restrict__ p, T* __restrict__ g, int64_t n8, int64_t i) {
  if (i >= n8) return;
  const vec8<T> gv = ((const vec8<T>*)g)[i];
  if (r.votes == 0.f) {
    ((vec8<T>*)p)[i] = gv;
    return;
  }
  const vec8<T> pv = ((const vec8<T>*)p)[i];
  const f32x8 sv = ((const f32x8*)bucket)[i];
  f32x8 hv = ((f32x8*)h)[i], lv = r.take ? ((f32x8*)lam)[i] : f32x8{}, xv;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float he = hv[e], le = lv[e];
    xv[e] = feddyn_elem<STEP>(r, sv[e], (float)pv[e], (float)gv[e], he, le);
    hv[e] = he;
    lv[e] = le;
  }
  if (r.take) ((f32x8*)lam)[i] = lv;
  if constexpr (STEP) ((f32x8*)h)[i] = hv;
  deliver8<T>(xv, p, g, i);
}

// both flat buffers in one launch, split as fedopt8_step_kernel splits them: blocks [0, nb16) the fp16 trainables
template <bool STEP>
__global__ void feddyn8_kernel(const float* __restrict__ bucket, float alpha, int num_clients, float* __restrict__ h,
                               float* __restrict__ lam, const int* __restrict__ flag, f16* __restrict__ p16,
                               int64_t n16, float* __restrict__ p32, int64_t n32, f16* __restrict__ g16,
                               float* __restrict__ g32, unsigned nb16) {
  const DynRound r = dyn_round<STEP>(bucket, n16 + n32, alpha, num_clients, flag);
  if (blockIdx.x < nb16)
    feddyn8_body<f16, STEP>(bucket, r, h, lam, p16, g16, n16 / 8, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  else
    feddyn8_body<float, STEP>(bucket + n16, r, h + n16, lam + n16, p32, g32, n32 / 8,
                              (int64_t)(blockIdx.x - nb16) * blockDim.x + threadIdx.x);
}

// out[i] = (((g_0[i] + g_1[i]) + g_2[i]) + ...) in client order, g_c = gathered + c * stride: the
// per-key torch.stack(...) sum of trainers/maple_fed.py:311-314 in the order the reference stacks its
// clients, whatever order the collective delivered them in (8 floats per thread, fp32 accumulation)
__global__ void reduce_ordered_kernel(const float* __restrict__ g, int nclients, int64_t stride, int64_t n,
                                      float* __restrict__ out) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n && stride % 4 == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)out % 16) == 0) {
    float4 acc = *(const float4*)(g + i);
    for (int c = 1; c < nclients; ++c) {
      const float4 v = *(const float4*)(g + (int64_t)c * stride + i);
      acc.x += v.x;
      acc.y += v.y;
      acc.z += v.z;
      acc.w += v.w;
    }
    *(float4*)(out + i) = acc;
  } else {
    for (int64_t j = i; j < n && j < i + 4; ++j) {
      float acc = g[j];
      for (int c = 1; c < nclients; ++c) acc += g[(int64_t)c * stride + j];
      out[j] = acc;
    }
  }
}

// Robust aggregation: the coordinate-wise median and beta-trimmed mean of Yin, Chen, Ramchandran, Bartlett
// ("Byzantine-Robust Distributed Learning: Towards Optimal Statistical Rates", ICML 2018) over the same
// [client][coordinate] image reduce_ordered_kernel sums.  Per coordinate (the contract of include/mapfed.h): a NaN is
// an absent client, the m present values are sorted in the IEEE total order, k = min(trim_k, (m - 1) / 2) are cut at
// either end, and the kept ones are summed in ascending order (one fp32 add each, starting from the first kept value)
// and divided by m - 2k.  A sum in sorted order depends on neither the client order nor the layout of the exchange.
//
// An absent client, and the padding of the client count to the network's size:
constexpr unsigned QUIET_NAN = 0x7fc00000u;

// the total order as a signed integer compare (an involution: the same expression turns a key back into its bits)
MF_DEV int order_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

// Batcher's odd-even merge sort on NP = 2^q keys as a list of compare-exchange pairs, built at compile time
// (NP = 8: 19 pairs, 64: 543), so the network below unrolls into min / max pairs on named registers: an index that is
// not a compile-time constant would send the key array to scratch.
template <int NP>
struct SortNet {
  int a[NP * 10], b[NP * 10], count;
};

template <int NP>
constexpr SortNet<NP> make_sort_net() {
  SortNet<NP> s{};
  for (int p = 1; p < NP; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < NP; j += 2 * k)
        for (int i = 0; i < k && i + j + k < NP; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            s.a[s.count] = i + j;
            s.b[s.count] = i + j + k;
            ++s.count;
          }
  return s;
}

template <int NP>
struct SortNetOf {
  static constexpr SortNet<NP> net = make_sort_net<NP>();
};

template <int A, int B, int NP>
MF_DEV void compare_exchange(unsigned (&key)[NP]) {
  const unsigned lo = min(key[A], key[B]), hi = max(key[A], key[B]);
  key[A] = lo;
  key[B] = hi;
}

template <int NP, size_t... T>
MF_DEV void sort_keys(unsigned (&key)[NP], std::index_sequence<T...>) {
  (compare_exchange<SortNetOf<NP>::net.a[T], SortNetOf<NP>::net.b[T]>(key), ...);
}

// one coordinate: key[] holds the NP raw bit patterns (the padding as NaNs) and is consumed.  The sort runs on
// u = order_key(bits) - order_key(-Inf) as an unsigned number: the present values keep their order in
// [0, U_INF], and every NaN, whatever its sign, wraps to above U_INF, so absent clients sort to the top untouched.
constexpr unsigned KEY_NINF = 0x807fffffu;         // order_key(bits of -Inf)
constexpr unsigned U_INF = 0x7f800000u - KEY_NINF;  // u of +Inf, the largest present value

template <int NP>
MF_DEV float trimmed_stat(unsigned (&key)[NP], int trim_k, bool is_count) {
  int m = 0;
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    key[c] = (unsigned)order_key((int)key[c]) - KEY_NINF;
    m += key[c] <= U_INF;
  }
  sort_keys<NP>(key, std::make_index_sequence<SortNetOf<NP>::net.count>{});
  // the present values now stand at [0, m); the kept range is [k, m - k).  A position outside it adds -0.f, the
  // identity of the fp32 add for every value (-0 included), and the accumulator starts as -0.f, so the sum is
  // s_k, then one add per further kept value: it starts from the first kept value, not from +0.
  const int k = m > 0 ? min(trim_k, (m - 1) >> 1) : 0;
  const unsigned kept = (unsigned)(m - 2 * k);
  float acc = -0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const float v = __int_as_float(order_key((int)(key[p] + KEY_NINF)));
    acc += (unsigned)(p - k) < kept ? v : -0.f;
  }
  if (is_count) return (float)m;
  return m > 0 ? acc / (float)kept : 0.f;
}

// Each thread owns VEC whole coordinates i .. i + VEC - 1 < n (the launcher sees to that): VEC = 4 with one 16-byte
// load per client, which needs stride % 4 == 0 and 16-byte aligned gathered / out, VEC = 1 with 4-byte loads; both
// are contiguous across the wave, and both run the same arithmetic per coordinate.
template <int NP, int VEC>
__global__ void __launch_bounds__(256)
    reduce_trimmed_kernel(const float* __restrict__ g, int nclients, int64_t stride, int64_t n, int trim_k,
                          int64_t count_pos, float* __restrict__ out) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (i >= n) return;
  if constexpr (VEC == 4) {
    unsigned k0[NP], k1[NP], k2[NP], k3[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) {
      k0[c] = k1[c] = k2[c] = k3[c] = QUIET_NAN;
      if (c < nclients) {
        const float4 v = *(const float4*)(g + (int64_t)c * stride + i);
        k0[c] = __float_as_uint(v.x);
        k1[c] = __float_as_uint(v.y);
        k2[c] = __float_as_uint(v.z);
        k3[c] = __float_as_uint(v.w);
      }
    }
    float4 r;
    r.x = trimmed_stat<NP>(k0, trim_k, count_pos == i);
    r.y = trimmed_stat<NP>(k1, trim_k, count_pos == i + 1);
    r.z = trimmed_stat<NP>(k2, trim_k, count_pos == i + 2);
    r.w = trimmed_stat<NP>(k3, trim_k, count_pos == i + 3);
    *(float4*)(out + i) = r;
  } else {
    unsigned key[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) {
      key[c] = QUIET_NAN;
      if (c < nclients) key[c] = __float_as_uint(g[(int64_t)c * stride + i]);
    }
    out[i] = trimmed_stat<NP>(key, trim_k, count_pos == i);
  }
}

// Up to 16 clients: four coordinates per thread over the multiple-of-4 part when the image allows 16-byte loads
// (4 * NP key registers), and the ragged tail, an unaligned image and 17 to 64 clients one coordinate per thread.
template <int NP>
void launch_reduce_trimmed(const float* g, int nclients, int64_t stride, int64_t n, int trim_k, int64_t count_pos,
                           float* out, hipStream_t st) {
  int64_t n4 = 0;
  if constexpr (NP <= 16) {
    if (stride % 4 == 0 && aligned(g, 16) && aligned(out, 16)) n4 = n & ~(int64_t)3;
    if (n4 > 0)
      reduce_trimmed_kernel<NP, 4><<<nblk(n4 / 4), 256, 0, st>>>(g, nclients, stride, n4, trim_k, count_pos, out);
  }
  if (n > n4)
    reduce_trimmed_kernel<NP, 1><<<nblk(n - n4), 256, 0, st>>>(g + n4, nclients, stride, n - n4, trim_k,
                                                              count_pos - n4, out + n4);
}

// flag[0] |= 1 if any element is NaN/Inf
__global__ void nonfinite_kernel(const void* __restrict__ x, int64_t n, int is16, int* __restrict__ flag) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = is16 ? (float)((const f16*)x)[i] : ((const float*)x)[i];
    bad |= !isfinite(v);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// clip_grad_norm_ in two launches: the per-chunk partial sums, then the coefficient.  With a non-null hyper the
// second also latches hyper[4] = max(hyper[4], *halt_src, *input_flag) for the SGD launch that follows (input_flag
// may be null)
int clip_launches(const void* g16, const float* g32, const void* chunks, int nchunks, float max_norm, float* part,
                  float* out, float* hyper, const float* halt_src, const int* input_flag, hipStream_t st) {
  if (nchunks > 0) {
    sumsq_chunks_kernel<<<nchunks, 256, 0, st>>>((const f16*)g16, g32, (const Chunk*)chunks, part);
    MF_CHECK_LAUNCH();
  }
  clip_coef_kernel<<<1, 1024, 0, st>>>(part, (const Chunk*)chunks, nchunks, max_norm, out, hyper, halt_src,
                                       input_flag);
  MF_CHECK_LAUNCH();
  return 0;
}

// SGD over one flat buffer: 8 elements per thread when the size and every pointer allow (a null pglob or lam does),
// one element per thread otherwise
template <int MODE>
int sgd_step(void* p, void* g, void* buf, const void* pglob, const float* lam, int64_t n, int is16, const float* coef,
             const float* hyper, hipStream_t st) {
  if (n <= 0) return 0;
  const bool vec = n % 8 == 0 && aligned(p, 32) && aligned(g, 32) && aligned(buf, 32) && aligned(pglob, 32) &&
                   aligned(lam, 32);
  if (vec && is16)
    sgd8_kernel<f16, MODE><<<nblk(n / 8), 256, 0, st>>>((f16*)p, (f16*)g, (f16*)buf, (const f16*)pglob, lam, n / 8,
                                                        coef, hyper);
  else if (vec)
    sgd8_kernel<float, MODE><<<nblk(n / 8), 256, 0, st>>>((float*)p, (float*)g, (float*)buf, (const float*)pglob, lam,
                                                          n / 8, coef, hyper);
  else if (is16)
    sgd_kernel<f16, MODE><<<nblk(n), 256, 0, st>>>((f16*)p, (f16*)g, (f16*)buf, (const f16*)pglob, lam, n, coef,
                                                   hyper);
  else
    sgd_kernel<float, MODE><<<nblk(n), 256, 0, st>>>((float*)p, (float*)g, (float*)buf, (const float*)pglob, lam, n,
                                                     coef, hyper);
  MF_CHECK_LAUNCH();
  return 0;
}

// The whole optimizer step in three launches: clip_launches (the latch replaces the two torch.maximum launches the
// engine used to make, at the step's start for the input check and here for the loss), then SGD over the fp16 and the
// fp32 flat buffers in one launch.  Bit-identical to mf_clip_grad_norm + two mf_sgd_step (SGD_PROX: mf_sgd_prox_step,
// SGD_DYN: mf_sgd_dyn_step; the clip norm is the model gradient's, without the proximal and the linear term).  lam
// (SGD_DYN; null otherwise) covers both buffers, [fp16 trainables | fp32 trainables]: lam + n16 is 32-byte aligned
// exactly when lam is and n16 % 8 == 0.
template <int MODE>
int optimizer_step(void* p16, void* g16, void* b16, const void* glob16, int64_t n16, float* p32, float* g32,
                   float* b32, const float* glob32, int64_t n32, const float* lam, const void* chunks, int nchunks,
                   float max_norm, float* part, float* out, float* hyper, const float* halt_src,
                   const int* input_flag, hipStream_t st) {
  int rc = clip_launches(g16, g32, chunks, nchunks, max_norm, part, out, hyper, halt_src, input_flag, st);
  if (rc) return rc;
  const float* lam32 = lam ? lam + n16 : nullptr;
  const bool vec16 = n16 % 8 == 0 && aligned(p16, 32) && aligned(g16, 32) && aligned(b16, 32) &&
                     aligned(glob16, 32) && aligned(lam, 32);
  const bool vec32 = n32 % 8 == 0 && aligned(p32, 32) && aligned(g32, 32) && aligned(b32, 32) &&
                     aligned(glob32, 32) && aligned(lam32, 32);
  if (vec16 && vec32 && n16 + n32 > 0) {
    const unsigned nb16 = nblk(n16 / 8), nb32 = nblk(n32 / 8);
    sgd8_both_kernel<MODE><<<nb16 + nb32, 256, 0, st>>>((f16*)p16, (f16*)g16, (f16*)b16, (const f16*)glob16, lam,
                                                        n16 / 8, p32, g32, b32, glob32, lam32, n32 / 8, nb16, out,
                                                        hyper);
    MF_CHECK_LAUNCH();
    return 0;
  }
  rc = sgd_step<MODE>(p16, g16, b16, glob16, lam, n16, 1, out, hyper, st);
  return rc ? rc : sgd_step<MODE>(p32, g32, b32, glob32, lam32, n32, 0, out, hyper, st);
}

template <bool WEIGHTED>
int fedavg_unpack(const float* bucket, void* p16, int64_t n16, float* p32, int64_t n32, void* g16, float* g32,
                  void* stream) {
  if (n16 + n32 <= 0) return 0;
  unpack_kernel<WEIGHTED><<<nblk(n16 + n32), 256, 0, (hipStream_t)stream>>>(bucket, (f16*)p16, n16, p32, n32,
                                                                            (f16*)g16, g32);
  MF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int mf_optim_chunk_bytes() { return (int)sizeof(Chunk); }
extern "C" int mf_optim_chunk_elems() { return CHUNK; }

// chunks: device array of Chunk {int seg, int is16, int64 start, int64 end}; part: nchunks floats;
// out: 3 floats (total norm, coef, finite flag)
extern "C" int mf_clip_grad_norm(const void* g16, const float* g32, const void* chunks, int nchunks, float max_norm,
                                 float* part, float* out, void* stream) {
  if (nchunks <= 0) return 0;
  return clip_launches(g16, g32, chunks, nchunks, max_norm, part, out, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int mf_sgd_step(void* p, void* g, void* buf, int64_t n, int is16, const float* coef, const float* hyper,
                           void* stream) {
  return sgd_step<SGD_PLAIN>(p, g, buf, nullptr, nullptr, n, is16, coef, hyper, (hipStream_t)stream);
}

// mf_sgd_step with the FedProx term mu * (p - pglob), mu = hyper[5] (a 6-float hyper)
extern "C" int mf_sgd_prox_step(void* p, void* g, void* buf, const void* pglob, int64_t n, int is16, const float* coef,
                                const float* hyper, void* stream) {
  if (n <= 0) return 0;
  if (!pglob) return mf_set_error("mf_sgd_prox_step: no global copy", -1);
  return sgd_step<SGD_PROX>(p, g, buf, pglob, nullptr, n, is16, coef, hyper, (hipStream_t)stream);
}

// mf_sgd_prox_step with FedDyn's linear term: alpha = hyper[5] in mu's place, then lam (n fp32 elements) subtracted
extern "C" int mf_sgd_dyn_step(void* p, void* g, void* buf, const void* pglob, const float* lam, int64_t n, int is16,
                               const float* coef, const float* hyper, void* stream) {
  if (n <= 0) return 0;
  if (!pglob) return mf_set_error("mf_sgd_dyn_step: no global copy", -1);
  if (!lam) return mf_set_error("mf_sgd_dyn_step: no lam", -1);
  return sgd_step<SGD_DYN>(p, g, buf, pglob, lam, n, is16, coef, hyper, (hipStream_t)stream);
}

extern "C" int mf_optimizer_step(void* p16, void* g16, void* b16, int64_t n16, float* p32, float* g32, float* b32,
                                 int64_t n32, const void* chunks, int nchunks, float max_norm, float* part, float* out,
                                 float* hyper, const float* halt_src, const int* input_flag, void* stream) {
  return optimizer_step<SGD_PLAIN>(p16, g16, b16, nullptr, n16, p32, g32, b32, nullptr, n32, nullptr, chunks, nchunks,
                                   max_norm, part, out, hyper, halt_src, input_flag, (hipStream_t)stream);
}

// mf_optimizer_step with the proximal SGD launch
extern "C" int mf_optimizer_step_prox(void* p16, void* g16, void* b16, int64_t n16, float* p32, float* g32, float* b32,
                                      int64_t n32, const void* chunks, int nchunks, float max_norm, float* part,
                                      float* out, float* hyper, const float* halt_src, const int* input_flag,
                                      const void* glob16, const float* glob32, void* stream) {
  if ((n16 > 0 && !glob16) || (n32 > 0 && !glob32)) return mf_set_error("mf_optimizer_step_prox: no global copy", -1);
  return optimizer_step<SGD_PROX>(p16, g16, b16, glob16, n16, p32, g32, b32, glob32, n32, nullptr, chunks, nchunks,
                                  max_norm, part, out, hyper, halt_src, input_flag, (hipStream_t)stream);
}

// mf_optimizer_step_prox with the dynamic SGD launch: lam, n16 + n32 fp32 elements in the bucket's order
extern "C" int mf_optimizer_step_dyn(void* p16, void* g16, void* b16, int64_t n16, float* p32, float* g32, float* b32,
                                     int64_t n32, const void* chunks, int nchunks, float max_norm, float* part,
                                     float* out, float* hyper, const float* halt_src, const int* input_flag,
                                     const void* glob16, const float* glob32, const float* lam, void* stream) {
  if ((n16 > 0 && !glob16) || (n32 > 0 && !glob32)) return mf_set_error("mf_optimizer_step_dyn: no global copy", -1);
  if (n16 + n32 > 0 && !lam) return mf_set_error("mf_optimizer_step_dyn: no lam", -1);
  return optimizer_step<SGD_DYN>(p16, g16, b16, glob16, n16, p32, g32, b32, glob32, n32, lam, chunks, nchunks, max_norm,
                                 part, out, hyper, halt_src, input_flag, (hipStream_t)stream);
}

extern "C" int mf_fedavg_pack(const void* p16, int64_t n16, const float* p32, int64_t n32, const int* invalid_flag,
                              float* bucket, void* stream) {
  if (n16 < 0 || n32 < 0) return mf_set_error("mf_fedavg_pack: negative size", -1);
  pack_kernel<false><<<nblk(n16 + n32 + TAIL<false>), 256, 0, (hipStream_t)stream>>>((const f16*)p16, n16, p32, n32,
                                                                                     invalid_flag, bucket, 1.f);
  MF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mf_fedavg_pack_weighted(const void* p16, int64_t n16, const float* p32, int64_t n32,
                                       const int* invalid_flag, float weight, float* bucket, void* stream) {
  if (n16 < 0 || n32 < 0) return mf_set_error("mf_fedavg_pack_weighted: negative size", -1);
  if (!(weight > 0.f) || __builtin_isinf(weight)) return mf_set_error("mf_fedavg_pack_weighted: weight not in (0, inf)", -1);
  pack_kernel<true><<<nblk(n16 + n32 + TAIL<true>), 256, 0, (hipStream_t)stream>>>((const f16*)p16, n16, p32, n32,
                                                                                   invalid_flag, bucket, weight);
  MF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mf_fedavg_unpack(const float* bucket, void* p16, int64_t n16, float* p32, int64_t n32, void* g16,
                                float* g32, void* stream) {
  return fedavg_unpack<false>(bucket, p16, n16, p32, n32, g16, g32, stream);
}

extern "C" int mf_fedavg_unpack_weighted(const float* bucket, void* p16, int64_t n16, float* p32, int64_t n32,
                                         void* g16, float* g32, void* stream) {
  return fedavg_unpack<true>(bucket, p16, n16, p32, n32, g16, g32, stream);
}

// The FedOpt server step on the summed bucket (weighted = 0: [sum | votes], 1: [sum | wsum | votes]), one launch
// over n16 + n32 elements.  opt: 1 fedavgm, 2 fedadagrad, 3 fedadam, 4 fedyogi; v is unused (may be null) for 1.
extern "C" int mf_fedopt_step(const float* bucket, int weighted, int opt, float beta1, float beta2, float tau,
                              float eta, float* x, float* m, float* v, void* p16, int64_t n16, float* p32,
                              int64_t n32, void* g16, float* g32, void* stream) {
  if (n16 < 0 || n32 < 0) return mf_set_error("mf_fedopt_step: negative size", -1);
  if (opt < FEDOPT_AVGM || opt > FEDOPT_YOGI) return mf_set_error("mf_fedopt_step: unknown optimizer id", -1);
  if (weighted != 0 && weighted != 1) return mf_set_error("mf_fedopt_step: weighted is 0 or 1", -1);
  const bool adaptive = opt != FEDOPT_AVGM;
  if (!__builtin_isfinite(beta1) || !__builtin_isfinite(beta2) || !__builtin_isfinite(tau) ||
      !__builtin_isfinite(eta))
    return mf_set_error("mf_fedopt_step: non-finite hyper-parameter", -1);
  if (adaptive && !(tau > 0.f)) return mf_set_error("mf_fedopt_step: tau <= 0 for an adaptive optimizer", -1);
  if (!x || !m || (adaptive && !v)) return mf_set_error("mf_fedopt_step: null state pointer", -1);
  if (n16 + n32 == 0) return 0;
  if (!bucket || (n16 > 0 && (!p16 || !g16)) || (n32 > 0 && (!p32 || !g32)))
    return mf_set_error("mf_fedopt_step: null bucket, weights or global copy", -1);
  hipStream_t st = (hipStream_t)stream;
  const FedOptHyper h{opt, beta1, beta2, tau, eta};
  const bool vec = n16 % 8 == 0 && n32 % 8 == 0 && aligned(bucket, 32) && aligned(x, 32) && aligned(m, 32) &&
                   (!adaptive || aligned(v, 32)) && aligned(p16, 16) && aligned(g16, 16) && aligned(p32, 32) &&
                   aligned(g32, 32);
  if (vec) {
    const unsigned nb16 = nblk(n16 / 8), nb32 = nblk(n32 / 8);
    fedopt8_step_kernel<<<nb16 + nb32, 256, 0, st>>>(bucket, weighted, h, x, m, adaptive ? v : nullptr, (f16*)p16, n16,
                                                     p32, n32, (f16*)g16, g32, nb16);
  } else {
    fedopt_step_kernel<<<nblk(n16 + n32), 256, 0, st>>>(bucket, weighted, h, x, m, v, (f16*)p16, n16, p32, n32,
                                                        (f16*)g16, g32);
  }
  MF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mf_fedopt_deliver(const float* x, void* p16, int64_t n16, float* p32, int64_t n32, void* g16,
                                 float* g32, void* stream) {
  if (n16 < 0 || n32 < 0) return mf_set_error("mf_fedopt_deliver: negative size", -1);
  if (!x) return mf_set_error("mf_fedopt_deliver: null state pointer", -1);
  if (n16 + n32 == 0) return 0;
  if ((n16 > 0 && (!p16 || !g16)) || (n32 > 0 && (!p32 || !g32)))
    return mf_set_error("mf_fedopt_deliver: null weights or global copy", -1);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = n16 % 8 == 0 && n32 % 8 == 0 && aligned(x, 32) && aligned(p16, 16) && aligned(g16, 16) &&
                   aligned(p32, 32) && aligned(g32, 32);
  if (vec) {
    const unsigned nb16 = nblk(n16 / 8), nb32 = nblk(n32 / 8);
    fedopt8_deliver_kernel<<<nb16 + nb32, 256, 0, st>>>(x, (f16*)p16, n16, p32, n32, (f16*)g16, g32, nb16);
  } else {
    fedopt_deliver_kernel<<<nblk(n16 + n32), 256, 0, st>>>(x, (f16*)p16, n16, p32, n32, (f16*)g16, g32);
  }
  MF_CHECK_LAUNCH();
  return 0;
}

namespace {

// the checks and the launch mf_feddyn_step and mf_feddyn_deliver share; launch shape as mf_fedopt_step's
template <bool STEP>
int feddyn_launch(const char* who, const float* bucket, float alpha, int num_clients, float* h, float* lam,
                  const int* flag, void* p16, int64_t n16, float* p32, int64_t n32, void* g16, float* g32,
                  hipStream_t st) {
  char msg[96];
  const auto fail = [&](const char* what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return mf_set_error(msg, -1);
  };
  if (n16 < 0 || n32 < 0) return fail("negative size");
  if (!__builtin_isfinite(alpha) || !(alpha > 0.f)) return fail("alpha not finite and > 0");
  if (num_clients < 1) return fail("num_clients < 1");
  if (!h || !lam || !flag) return fail("null h, lam or flag");
  if (n16 + n32 == 0) return 0;
  if (!bucket || (n16 > 0 && (!p16 || !g16)) || (n32 > 0 && (!p32 || !g32)))
    return fail("null bucket, weights or global copy");
  const bool vec = n16 % 8 == 0 && n32 % 8 == 0 && aligned(bucket, 32) && aligned(h, 32) && aligned(lam, 32) &&
                   aligned(p16, 16) && aligned(g16, 16) && aligned(p32, 32) && aligned(g32, 32);
  if (vec) {
    const unsigned nb16 = nblk(n16 / 8), nb32 = nblk(n32 / 8);
    feddyn8_kernel<STEP><<<nb16 + nb32, 256, 0, st>>>(bucket, alpha, num_clients, h, lam, flag, (f16*)p16, n16, p32,
                                                      n32, (f16*)g16, g32, nb16);
  } else {
    feddyn_kernel<STEP><<<nblk(n16 + n32), 256, 0, st>>>(bucket, alpha, num_clients, h, lam, flag, (f16*)p16, n16, p32,
                                                         n32, (f16*)g16, g32);
  }
  MF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// FedDyn's round end on the summed plain bucket [sum | votes]: the server's h steps, this client's lam updates (unless
// *flag) and x = mean - h / alpha is delivered as fp16 into its weights and global copy
extern "C" int mf_feddyn_step(const float* bucket, float alpha, int num_clients, float* h, float* lam, const int* flag,
                              void* p16, int64_t n16, float* p32, int64_t n32, void* g16, float* g32, void* stream) {
  return feddyn_launch<true>("mf_feddyn_step", bucket, alpha, num_clients, h, lam, flag, p16, n16, p32, n32, g16, g32,
                             (hipStream_t)stream);
}

// ... for the rank's second and later clients: the stepped h is only read, the same x recomputed, this client's own lam
// updated from its own weights and global copy
extern "C" int mf_feddyn_deliver(const float* bucket, float alpha, const float* h, float* lam, const int* flag,
                                 void* p16, int64_t n16, float* p32, int64_t n32, void* g16, float* g32,
                                 void* stream) {
  return feddyn_launch<false>("mf_feddyn_deliver", bucket, alpha, 1, (float*)h, lam, flag, p16, n16, p32, n32, g16,
                              g32, (hipStream_t)stream);
}

extern "C" int mf_fedavg_reduce_ordered(const float* gathered, int nclients, int64_t stride, int64_t n, float* out,
                                        void* stream) {
  if (nclients < 1 || n < 0 || stride < n) return mf_set_error("mf_fedavg_reduce_ordered: bad sizes", -1);
  if (n == 0) return 0;
  reduce_ordered_kernel<<<nblk((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(gathered, nclients, stride, n, out);
  MF_CHECK_LAUNCH();
  return 0;
}

// The robust aggregation's reduce in mf_fedavg_reduce_ordered's place (same image); median = a large trim_k
extern "C" int mf_fedavg_reduce_trimmed(const float* gathered, int nclients, int64_t stride, int64_t n, int trim_k,
                                        int64_t count_pos, float* out, void* stream) {
  if (nclients < 1 || nclients > 64) return mf_set_error("mf_fedavg_reduce_trimmed: nclients not in [1, 64]", -1);
  if (trim_k < 0) return mf_set_error("mf_fedavg_reduce_trimmed: trim_k < 0", -1);
  if (n < 0 || stride < n) return mf_set_error("mf_fedavg_reduce_trimmed: bad sizes (n < 0 or stride < n)", -1);
  if (count_pos >= n) return mf_set_error("mf_fedavg_reduce_trimmed: count_pos >= n", -1);
  if (n == 0) return 0;
  if (!gathered || !out) return mf_set_error("mf_fedavg_reduce_trimmed: null pointer", -1);
  hipStream_t st = (hipStream_t)stream;
  if (nclients <= 2)
    launch_reduce_trimmed<2>(gathered, nclients, stride, n, trim_k, count_pos, out, st);
  else if (nclients <= 4)
    launch_reduce_trimmed<4>(gathered, nclients, stride, n, trim_k, count_pos, out, st);
  else if (nclients <= 8)
    launch_reduce_trimmed<8>(gathered, nclients, stride, n, trim_k, count_pos, out, st);
  else if (nclients <= 16)
    launch_reduce_trimmed<16>(gathered, nclients, stride, n, trim_k, count_pos, out, st);
  else if (nclients <= 32)
    launch_reduce_trimmed<32>(gathered, nclients, stride, n, trim_k, count_pos, out, st);
  else
    launch_reduce_trimmed<64>(gathered, nclients, stride, n, trim_k, count_pos, out, st);
  MF_CHECK_LAUNCH();
  return 0;
}

// The robust aggregation's bucket: mf_fedavg_pack_weighted's layout at weight 1, an invalid client all quiet NaNs
extern "C" int mf_fedavg_pack_robust(const void* p16, int64_t n16, const float* p32, int64_t n32,
                                     const int* invalid_flag, float* bucket, void* stream) {
  if (n16 < 0 || n32 < 0) return mf_set_error("mf_fedavg_pack_robust: negative size", -1);
  pack_kernel<true, true><<<nblk(n16 + n32 + TAIL<true>), 256, 0, (hipStream_t)stream>>>(
      (const f16*)p16, n16, p32, n32, invalid_flag, bucket, 1.f);
  MF_CHECK_LAUNCH();
  return 0;
}

// DP-FedAvg's pack: the client's update clipped by *scale_ptr (mf_dp_update_scale's out + 1), in the bucket layout
// `layout` (0 plain, 1 weighted, 2 robust); with *scale_ptr >= 1 the bits of the three entry points above
extern "C" int mf_fedavg_pack_clipped(const void* p16, int64_t n16, const float* p32, int64_t n32, const void* g16,
                                      const float* g32, const int* invalid_flag, const float* scale_ptr, float weight,
                                      int layout, float* bucket, void* stream) {
  if (n16 < 0 || n32 < 0) return mf_set_error("mf_fedavg_pack_clipped: negative size", -1);
  if (layout < 0 || layout > 2) return mf_set_error("mf_fedavg_pack_clipped: layout is 0, 1 or 2", -1);
  if (layout == 1 && (!(weight > 0.f) || __builtin_isinf(weight)))
    return mf_set_error("mf_fedavg_pack_clipped: weight not in (0, inf)", -1);
  if (!scale_ptr) return mf_set_error("mf_fedavg_pack_clipped: null scale pointer", -1);
  if (!bucket || (n16 > 0 && (!p16 || !g16)) || (n32 > 0 && (!p32 || !g32)))
    return mf_set_error("mf_fedavg_pack_clipped: null bucket, weights or global copy", -1);
  hipStream_t st = (hipStream_t)stream;
  const f16 *p = (const f16*)p16, *g = (const f16*)g16;
  if (layout == 0)
    pack_kernel<false, false, true><<<nblk(n16 + n32 + TAIL<false>), 256, 0, st>>>(p, n16, p32, n32, invalid_flag,
                                                                                  bucket, 1.f, g, g32, scale_ptr);
  else if (layout == 1)
    pack_kernel<true, false, true><<<nblk(n16 + n32 + TAIL<true>), 256, 0, st>>>(p, n16, p32, n32, invalid_flag,
                                                                                bucket, weight, g, g32, scale_ptr);
  else
    pack_kernel<true, true, true><<<nblk(n16 + n32 + TAIL<true>), 256, 0, st>>>(p, n16, p32, n32, invalid_flag, bucket,
                                                                               1.f, g, g32, scale_ptr);
  MF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mf_nonfinite_flag(const void* x, int64_t n, int is16, int* flag, void* stream) {
  if (n <= 0) return 0;
  unsigned g = nblk(n);
  if (g > 2048) g = 2048;
  nonfinite_kernel<<<g, 256, 0, (hipStream_t)stream>>>(x, n, is16, flag);
  MF_CHECK_LAUNCH();
  return 0;
}
