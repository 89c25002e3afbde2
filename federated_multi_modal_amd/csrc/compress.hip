// int8 compression of the FedAvg uplink with error feedback: the client's update w_k - g against the round's starting
// weights, one shared fp32 scale per block of 256 coordinates, rounded to nearest or stochastically (QSGD: Alistarh,
// Grubic, Li, Tomioka, Vojnovic, NeurIPS 2017), the rounding error kept in a per-client residual (Seide et al. 2014;
// Karimireddy, Rebjock, Stich, Jaggi, ICML 2019).  The quantiser writes the wire chunks of the exchange's send image
// itself; the decoder rebuilds the fp32 image the reduce kernels of optim.hip read.  The contract is in
// include/mapfed.h.
//
// Every fp32 operation below is rounded on its own (no fused multiply-add), no float atomics, and every store is a
// plain vector store.
#include "mf_common.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace {

constexpr int QB = 256;  // coordinates per quantisation block: one wave64, four per lane

// coordinate i of [fp16 buffer | fp32 buffer], 0 at and past n
MF_DEV float coord(const f16* __restrict__ a16, const float* __restrict__ a32, int64_t n16, int64_t n, int64_t i) {
  return i < n16 ? (float)a16[i] : (i < n ? a32[i - n16] : 0.f);
}

// coordinates i0 .. i0 + 3: one 8-byte load inside the fp16 buffer, one 16-byte load inside the fp32 buffer, where the
// address allows it; element loads across the boundary, past n and at any other address
MF_DEV void load4(const f16* __restrict__ a16, const float* __restrict__ a32, int64_t n16, int64_t n, int64_t i0,
                  float (&v)[4]) {
  if (i0 + 4 <= n16 && ((uintptr_t)(a16 + i0) & 7) == 0) {
    const f16x4 h = *(const f16x4*)(a16 + i0);
#pragma unroll
    for (int l = 0; l < 4; ++l) v[l] = (float)h[l];
  } else if (i0 >= n16 && i0 + 4 <= n && ((uintptr_t)(a32 + (i0 - n16)) & 15) == 0) {
    const f32x4 f = *(const f32x4*)(a32 + (i0 - n16));
#pragma unroll
    for (int l = 0; l < 4; ++l) v[l] = f[l];
  } else {
#pragma unroll
    for (int l = 0; l < 4; ++l) v[l] = coord(a16, a32, n16, n, i0 + l);
  }
}

// One wave per quantisation block, lane l its coordinates 256 * blk + 4 * l .. + 3: exactly the Philox counter
// 64 * blk + l.  S is a multiple of 256, so a block lies in one destination rank's chunk.
__global__ __launch_bounds__(256) void quantize_kernel(
    const f16* __restrict__ x16, const f16* __restrict__ g16, int64_t n16, const float* __restrict__ x32,
    const float* __restrict__ g32, int64_t n, const float* __restrict__ e_in, float* __restrict__ e_out,
    const int* __restrict__ invalid_flag, float weight, int stochastic, uint32_t k0, uint32_t k1, uint32_t round,
    uint32_t cword, uint8_t* __restrict__ image, int64_t rank_stride, int64_t S, int64_t nblocks) {
  const int lane = threadIdx.x & 63;
  const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= nblocks) return;  // the whole wave
  const int64_t i0 = blk * QB + 4 * lane;
  const int64_t r = (blk * QB) / S, j0 = i0 - r * S;
  uint8_t* chunk = image + r * rank_stride;
  const bool bad = invalid_flag != nullptr && *invalid_flag != 0;
  const bool e_vec = i0 + 4 <= n;

  float ev[4] = {0.f, 0.f, 0.f, 0.f};
  if (e_in) {
    if (e_vec && ((uintptr_t)(e_in + i0) & 15) == 0) {
      const f32x4 f = *(const f32x4*)(e_in + i0);
#pragma unroll
      for (int l = 0; l < 4; ++l) ev[l] = f[l];
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (i0 + l < n) ev[l] = e_in[i0 + l];
    }
  }

  float q[4] = {0.f, 0.f, 0.f, 0.f}, en[4], scale = 0.f;
  if (bad) {  // codes 0, scale 0, the residual carried over; no weight is read
#pragma unroll
    for (int l = 0; l < 4; ++l) en[l] = ev[l];
  } else {
    float xv[4], gv[4], u[4];
    load4(x16, x32, n16, n, i0, xv);
    load4(g16, g32, n16, n, i0, gv);
    float amax = 0.f;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const float d = xv[l] - gv[l];
      u[l] = e_in ? d + ev[l] : d;
      amax = fmaxf(amax, fabsf(u[l]));
    }
    amax = wave_max(amax);
    scale = amax / 127.0f;
    if (amax == 0.f) {
#pragma unroll
      for (int l = 0; l < 4; ++l) en[l] = u[l];
    } else {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (stochastic) {
        const uint64_t ctr = (uint64_t)i0 >> 2;
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), round, cword, k0, k1, w);
      }
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const float t = u[l] / scale;
        float qq;
        if (stochastic) {
          const float f = floorf(t);
          const float p = t - f;
          const float rr = (float)(w[l] >> 8) * 0x1p-24f;
          qq = f + (rr < p ? 1.f : 0.f);
        } else {
          qq = rintf(t);
        }
        qq = fminf(fmaxf(qq, -127.f), 127.f);  // finite from here on, whatever t was
        q[l] = qq;
        const float sq = scale * qq;
        en[l] = u[l] - sq;
      }
    }
  }

  uint32_t packed = 0u;
#pragma unroll
  for (int l = 0; l < 4; ++l) packed |= ((uint32_t)(int)q[l] & 0xffu) << (8 * l);
  *(uint32_t*)(chunk + j0) = packed;
  if (lane == 0) {
    *(float*)(chunk + S + 4 * (j0 / QB)) = scale;
    if (j0 == 0) {  // the tail, in every destination rank's chunk
      float* tail = (float*)(chunk + S + S / 64);
      tail[0] = bad ? 0.f : weight;
      tail[1] = bad ? 0.f : 1.f;
    }
  }
  if (e_out) {
    if (e_vec && ((uintptr_t)(e_out + i0) & 15) == 0) {
      f32x4 f;
#pragma unroll
      for (int l = 0; l < 4; ++l) f[l] = en[l];
      *(f32x4*)(e_out + i0) = f;
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (i0 + l < n) e_out[i0 + l] = en[l];
    }
  }
}

// blockIdx.y: the chunk (client); one thread per four coordinates j0 .. j0 + 3 of its shard, the global coordinates
// first + c * first_step + j
__global__ __launch_bounds__(256) void decode_kernel(const uint8_t* __restrict__ image, int64_t chunk_stride, int64_t S,
                                                     int64_t first, int64_t first_step, const f16* __restrict__ g16,
                                                     int64_t n16, const float* __restrict__ g32, int64_t n, int layout,
                                                     float* __restrict__ out, int64_t out_stride) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= S / 4) return;
  const int64_t c = blockIdx.y;
  const uint8_t* chunk = image + c * chunk_stride;
  const int64_t j0 = 4 * t, i0 = first + c * first_step + j0;
  const float* tail = (const float*)(chunk + S + S / 64);
  const float w = tail[0], vote = tail[1];
  float y[4];
  if (vote == 0.f) {  // an invalid client: what the pack kernels write for it
    const float fill = layout == 2 ? __uint_as_float(0x7fc00000u) : 0.f;
#pragma unroll
    for (int l = 0; l < 4; ++l) y[l] = fill;
  } else {
    const uint32_t codes = *(const uint32_t*)(chunk + j0);
    const float scale = *(const float*)(chunk + S + 4 * (j0 / QB));
    float gv[4];
    load4(g16, g32, n16, n, i0, gv);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int64_t i = i0 + l;
      if (i < n) {
        const float qf = (float)(int)(int8_t)(codes >> (8 * l));
        const float sq = scale * qf;
        const float yy = gv[l] + sq;
        y[l] = layout == 1 ? w * yy : yy;
      } else if (i == n) {
        y[l] = layout == 0 ? vote : w;
      } else if (i == n + 1 && layout != 0) {
        y[l] = vote;
      } else {
        y[l] = 0.f;
      }
    }
  }
  float* o = out + c * out_stride + j0;
  if (((uintptr_t)o & 15) == 0) {
    f32x4 f;
#pragma unroll
    for (int l = 0; l < 4; ++l) f[l] = y[l];
    *(f32x4*)o = f;
  } else {
#pragma unroll
    for (int l = 0; l < 4; ++l) o[l] = y[l];
  }
}

// ---- block-wise top-k of the same update, with the same error feedback (Aji & Heafield, EMNLP 2017; Stich, Cordonnier,
// Jaggi, NeurIPS 2018): from every block of 256 coordinates the k of largest magnitude travel as (uint8 index, fp32
// value), the others stay in the residual.  Chunk: [nb * k fp32 values | nb * k uint8 indices | zero bytes to a multiple
// of 4 | fp32 weight | fp32 vote], nb = S / 256.

MF_DEV int64_t topk_index_bytes(int64_t nbk) { return (nbk + 3) / 4 * 4; }

// One wave per block, lane l its coordinates 256 * blk + 4 * l .. + 3, as the quantiser.  The key of a coordinate is
// (|u| bits << 8) | (255 - index in the block): 39 bits, distinct within the block, so the k largest keys are the k
// largest magnitudes with ties going to the lower index.  The k-th largest key is found most significant bit first:
// a bit stays set when at least k keys reach the candidate, each count four ballots and their popcounts, 39 steps
// whatever k.  The output position of a kept coordinate is the number of kept coordinates before it.
__global__ __launch_bounds__(256) void topk_select_kernel(
    const f16* __restrict__ x16, const f16* __restrict__ g16, int64_t n16, const float* __restrict__ x32,
    const float* __restrict__ g32, int64_t n, const float* __restrict__ e_in, float* __restrict__ e_out,
    const int* __restrict__ invalid_flag, float weight, int k, uint8_t* __restrict__ image, int64_t rank_stride,
    int64_t S, int64_t nblocks) {
  const int lane = threadIdx.x & 63;
  const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= nblocks) return;  // the whole wave
  const int64_t i0 = blk * QB + 4 * lane;
  const int64_t nb = S / QB, r = blk / nb, bj = blk - r * nb;
  uint8_t* chunk = image + r * rank_stride;
  float* vals = (float*)chunk + bj * k;
  uint8_t* idx = chunk + 4 * nb * k + bj * k;
  const bool bad = invalid_flag != nullptr && *invalid_flag != 0;
  const bool e_vec = i0 + 4 <= n;

  float ev[4] = {0.f, 0.f, 0.f, 0.f};
  if (e_in) {
    if (e_vec && ((uintptr_t)(e_in + i0) & 15) == 0) {
      const f32x4 f = *(const f32x4*)(e_in + i0);
#pragma unroll
      for (int l = 0; l < 4; ++l) ev[l] = f[l];
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (i0 + l < n) ev[l] = e_in[i0 + l];
    }
  }

  float en[4];
  if (bad) {  // k zero entries, the residual carried over; no weight is read
#pragma unroll
    for (int l = 0; l < 4; ++l) en[l] = ev[l];
    if (lane < k) {
      vals[lane] = 0.f;
      idx[lane] = 0;
    }
  } else {
    float xv[4], gv[4], u[4];
    load4(x16, x32, n16, n, i0, xv);
    load4(g16, g32, n16, n, i0, gv);
    uint64_t key[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const float d = xv[l] - gv[l];
      u[l] = e_in ? d + ev[l] : d;
      key[l] = ((uint64_t)(__float_as_uint(u[l]) & 0x7fffffffu) << 8) | (uint32_t)(255 - (4 * lane + l));
    }
    uint64_t kth = 0;  // wave-uniform
    for (int b = 38; b >= 0; --b) {
      const uint64_t cand = kth | (1ull << b);
      int c = 0;
#pragma unroll
      for (int l = 0; l < 4; ++l) c += __popcll(__ballot(key[l] >= cand));
      if (c >= k) kth = cand;
    }
    bool kept[4];
    int pos = 0;  // kept coordinates of the lower lanes
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      kept[l] = key[l] >= kth;
      const uint64_t m = __ballot(kept[l]);
      pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      en[l] = kept[l] ? 0.f : u[l];
      if (kept[l]) {
        vals[pos] = u[l];
        idx[pos] = (uint8_t)(4 * lane + l);
        ++pos;
      }
    }
  }

  if (lane == 0) {
    if (bj == nb - 1) {  // the index region's padding
      for (int64_t p = nb * k; p < topk_index_bytes(nb * k); ++p) chunk[4 * nb * k + p] = 0;
    }
    if (bj == 0) {  // the tail, in every destination rank's chunk
      float* tail = (float*)(chunk + 4 * nb * k + topk_index_bytes(nb * k));
      tail[0] = bad ? 0.f : weight;
      tail[1] = bad ? 0.f : 1.f;
    }
  }
  if (e_out) {
    if (e_vec && ((uintptr_t)(e_out + i0) & 15) == 0) {
      f32x4 f;
#pragma unroll
      for (int l = 0; l < 4; ++l) f[l] = en[l];
      *(f32x4*)(e_out + i0) = f;
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (i0 + l < n) e_out[i0 + l] = en[l];
    }
  }
}

// blockIdx.y: the chunk (client); one wave per block of its shard, the global coordinates first + c * first_step + j.
// The wave clears its 1 KB tile of LDS, the lanes below k scatter their entry into it (the index is a byte: it cannot
// leave the tile), and every lane reads back its four coordinates.
__global__ __launch_bounds__(256) void topk_decode_kernel(const uint8_t* __restrict__ image, int64_t chunk_stride,
                                                          int64_t S, int64_t first, int64_t first_step,
                                                          const f16* __restrict__ g16, int64_t n16,
                                                          const float* __restrict__ g32, int64_t n, int layout, int k,
                                                          float* __restrict__ out, int64_t out_stride) {
  __shared__ __attribute__((aligned(16))) float tile[4][QB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nb = S / QB, bj = (int64_t)blockIdx.x * 4 + wave;
  const bool live = bj < nb;  // per wave; every wave reaches the barriers
  const int64_t c = blockIdx.y;
  const uint8_t* chunk = image + c * chunk_stride;
  const float* tail = (const float*)(chunk + 4 * nb * k + topk_index_bytes(nb * k));
  const float w = tail[0], vote = tail[1];  // uniform over the workgroup
  const bool sent = live && vote != 0.f;
  *(f32x4*)&tile[wave][4 * lane] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  if (sent && lane < k) tile[wave][chunk[4 * nb * k + bj * k + lane]] = ((const float*)chunk)[bj * k + lane];
  __syncthreads();
  if (!live) return;
  const int64_t j0 = bj * QB + 4 * lane, i0 = first + c * first_step + j0;
  float y[4] = {0.f, 0.f, 0.f, 0.f};
  if (sent) {  // vote 0, an invalid client: zeros, what the pack kernels write for it
    const f32x4 sv = *(const f32x4*)&tile[wave][4 * lane];
    float gv[4];
    load4(g16, g32, n16, n, i0, gv);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int64_t i = i0 + l;
      if (i < n) {
        const float yy = gv[l] + sv[l];
        y[l] = layout == 1 ? w * yy : yy;
      } else if (i == n) {
        y[l] = layout == 0 ? vote : w;
      } else if (i == n + 1 && layout != 0) {
        y[l] = vote;
      }
    }
  }
  float* o = out + c * out_stride + j0;
  if (((uintptr_t)o & 15) == 0) {
    f32x4 f;
#pragma unroll
    for (int l = 0; l < 4; ++l) f[l] = y[l];
    *(f32x4*)o = f;
  } else {
#pragma unroll
    for (int l = 0; l < 4; ++l) o[l] = y[l];
  }
}

}  // namespace

// bytes of one wire chunk of shard length S: [S int8 codes | S / 256 fp32 scales | fp32 weight | fp32 vote]
extern "C" int64_t mf_compress_chunk_bytes(int64_t S) {
  if (S <= 0 || S % QB != 0) return -1;
  return S + S / 64 + 8;
}

extern "C" int mf_compress_quantize(const void* x16, const void* g16, int64_t n16, const float* x32, const float* g32,
                                    int64_t n32, const float* e_in, float* e_out, const int* invalid_flag,
                                    float weight, int rounding, uint64_t seed, uint32_t round, uint32_t client,
                                    void* image, int64_t rank_stride, int64_t S, int world, void* stream) {
  if (n16 < 0 || n32 < 0) return mf_set_error("mf_compress_quantize: negative size", -1);
  if (S <= 0 || S % QB != 0) return mf_set_error("mf_compress_quantize: S not a positive multiple of 256", -1);
  if (world < 1) return mf_set_error("mf_compress_quantize: world < 1", -1);
  if (S > INT64_MAX / world || n16 > INT64_MAX - n32 || n16 + n32 > (int64_t)world * S)
    return mf_set_error("mf_compress_quantize: world * S shorter than n16 + n32", -1);
  if (rounding != 0 && rounding != 1) return mf_set_error("mf_compress_quantize: unknown rounding", -1);
  if (!(weight > 0.f) || __builtin_isinf(weight))
    return mf_set_error("mf_compress_quantize: weight not finite and > 0", -1);
  if (client >= 0x80000000u) return mf_set_error("mf_compress_quantize: client index above 2^31 - 1", -1);
  if (!image || !invalid_flag) return mf_set_error("mf_compress_quantize: null image or flag", -1);
  if ((n16 > 0 && (!x16 || !g16)) || (n32 > 0 && (!x32 || !g32)))
    return mf_set_error("mf_compress_quantize: null weights or global copy", -1);
  if ((e_in == nullptr) != (e_out == nullptr) || (e_in && e_in == e_out))
    return mf_set_error("mf_compress_quantize: residual in and out: both or neither, and two buffers", -1);
  const int64_t chunk = S + S / 64 + 8;
  if ((uintptr_t)image % 4 != 0 || rank_stride % 4 != 0 || (world > 1 && rank_stride < chunk))
    return mf_set_error("mf_compress_quantize: image or rank stride misaligned, or stride below a chunk", -1);
  const int64_t nblocks = (int64_t)world * (S / QB);
  if ((nblocks + 3) / 4 > 0x7fffffff) return mf_set_error("mf_compress_quantize: too large for one launch", -1);
  quantize_kernel<<<(unsigned)((nblocks + 3) / 4), 256, 0, (hipStream_t)stream>>>(
      (const f16*)x16, (const f16*)g16, n16, x32, g32, n16 + n32, e_in, e_out, invalid_flag, weight, rounding,
      (uint32_t)seed, (uint32_t)(seed >> 32), round, 0x80000000u | client, (uint8_t*)image, rank_stride, S, nblocks);
  MF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mf_compress_decode(const void* image, int64_t chunk_stride, int nclients, int64_t S, int64_t first,
                                  int64_t first_step, const void* g16, int64_t n16, const float* g32, int64_t n32,
                                  int layout, float* out, int64_t out_stride, void* stream) {
  if (n16 < 0 || n32 < 0 || first < 0 || first_step < 0)
    return mf_set_error("mf_compress_decode: negative size, first or first_step", -1);
  if (S <= 0 || S % QB != 0) return mf_set_error("mf_compress_decode: S not a positive multiple of 256", -1);
  if (nclients < 1 || nclients > 65535) return mf_set_error("mf_compress_decode: nclients outside 1..65535", -1);
  if (layout < 0 || layout > 2) return mf_set_error("mf_compress_decode: unknown layout", -1);
  if (!image || !out) return mf_set_error("mf_compress_decode: null image or out", -1);
  if ((n16 > 0 && !g16) || (n32 > 0 && !g32)) return mf_set_error("mf_compress_decode: null global copy", -1);
  const int64_t chunk = S + S / 64 + 8;
  if ((uintptr_t)image % 4 != 0 || chunk_stride % 4 != 0 || (nclients > 1 && (chunk_stride < chunk || out_stride < S)))
    return mf_set_error("mf_compress_decode: image or stride misaligned, or a stride below its element", -1);
  if ((uintptr_t)out % 4 != 0) return mf_set_error("mf_compress_decode: out not 4-byte aligned", -1);
  if (n16 > INT64_MAX - n32 || first_step > (INT64_MAX - first - S) / nclients)
    return mf_set_error("mf_compress_decode: coordinates overflow", -1);
  const int64_t bx = (S / 4 + 255) / 256;
  if (bx > 0x7fffffff) return mf_set_error("mf_compress_decode: S too large for one launch", -1);
  decode_kernel<<<dim3((unsigned)bx, (unsigned)nclients), 256, 0, (hipStream_t)stream>>>(
      (const uint8_t*)image, chunk_stride, S, first, first_step, (const f16*)g16, n16, g32, n16 + n32, layout, out,
      out_stride);
  MF_CHECK_LAUNCH();
  return 0;
}

// bytes of one top-k wire chunk of shard length S: [nb * k fp32 values | nb * k uint8 indices | zero bytes to a multiple
// of 4 | fp32 weight | fp32 vote], nb = S / 256
extern "C" int64_t mf_topk_chunk_bytes(int64_t S, int k) {
  if (S <= 0 || S % QB != 0 || k < 1 || k > 64) return -1;
  const int64_t nbk = S / QB * k;
  return 4 * nbk + (nbk + 3) / 4 * 4 + 8;
}

extern "C" int mf_topk_select(const void* x16, const void* g16, int64_t n16, const float* x32, const float* g32,
                              int64_t n32, const float* e_in, float* e_out, const int* invalid_flag, float weight, int k,
                              void* image, int64_t rank_stride, int64_t S, int world, void* stream) {
  if (n16 < 0 || n32 < 0) return mf_set_error("mf_topk_select: negative size", -1);
  if (S <= 0 || S % QB != 0) return mf_set_error("mf_topk_select: S not a positive multiple of 256", -1);
  if (k < 1 || k > 64) return mf_set_error("mf_topk_select: k outside 1..64", -1);
  if (world < 1) return mf_set_error("mf_topk_select: world < 1", -1);
  if (S > INT64_MAX / world || n16 > INT64_MAX - n32 || n16 + n32 > (int64_t)world * S)
    return mf_set_error("mf_topk_select: world * S shorter than n16 + n32", -1);
  if (!(weight > 0.f) || __builtin_isinf(weight)) return mf_set_error("mf_topk_select: weight not finite and > 0", -1);
  if (!image || !invalid_flag) return mf_set_error("mf_topk_select: null image or flag", -1);
  if ((n16 > 0 && (!x16 || !g16)) || (n32 > 0 && (!x32 || !g32)))
    return mf_set_error("mf_topk_select: null weights or global copy", -1);
  if ((e_in == nullptr) != (e_out == nullptr) || (e_in && e_in == e_out))
    return mf_set_error("mf_topk_select: residual in and out: both or neither, and two buffers", -1);
  const int64_t chunk = mf_topk_chunk_bytes(S, k);
  if ((uintptr_t)image % 4 != 0 || rank_stride % 4 != 0 || (world > 1 && rank_stride < chunk))
    return mf_set_error("mf_topk_select: image or rank stride misaligned, or stride below a chunk", -1);
  const int64_t nblocks = (int64_t)world * (S / QB);
  if ((nblocks + 3) / 4 > 0x7fffffff) return mf_set_error("mf_topk_select: too large for one launch", -1);
  topk_select_kernel<<<(unsigned)((nblocks + 3) / 4), 256, 0, (hipStream_t)stream>>>(
      (const f16*)x16, (const f16*)g16, n16, x32, g32, n16 + n32, e_in, e_out, invalid_flag, weight, k, (uint8_t*)image,
      rank_stride, S, nblocks);
  MF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mf_topk_decode(const void* image, int64_t chunk_stride, int nclients, int64_t S, int64_t first,
                              int64_t first_step, const void* g16, int64_t n16, const float* g32, int64_t n32, int layout,
                              float* out, int64_t out_stride, int k, void* stream) {
  if (n16 < 0 || n32 < 0 || first < 0 || first_step < 0)
    return mf_set_error("mf_topk_decode: negative size, first or first_step", -1);
  if (S <= 0 || S % QB != 0) return mf_set_error("mf_topk_decode: S not a positive multiple of 256", -1);
  if (k < 1 || k > 64) return mf_set_error("mf_topk_decode: k outside 1..64", -1);
  if (nclients < 1 || nclients > 65535) return mf_set_error("mf_topk_decode: nclients outside 1..65535", -1);
  if (layout < 0 || layout > 1) return mf_set_error("mf_topk_decode: unknown layout (plain and weighted only)", -1);
  if (!image || !out) return mf_set_error("mf_topk_decode: null image or out", -1);
  if ((n16 > 0 && !g16) || (n32 > 0 && !g32)) return mf_set_error("mf_topk_decode: null global copy", -1);
  const int64_t chunk = mf_topk_chunk_bytes(S, k);
  if ((uintptr_t)image % 4 != 0 || chunk_stride % 4 != 0 || (nclients > 1 && (chunk_stride < chunk || out_stride < S)))
    return mf_set_error("mf_topk_decode: image or stride misaligned, or a stride below its element", -1);
  if ((uintptr_t)out % 4 != 0) return mf_set_error("mf_topk_decode: out not 4-byte aligned", -1);
  if (n16 > INT64_MAX - n32 || first_step > (INT64_MAX - first - S) / nclients)
    return mf_set_error("mf_topk_decode: coordinates overflow", -1);
  const int64_t bx = (S / QB + 3) / 4;
  if (bx > 0x7fffffff) return mf_set_error("mf_topk_decode: S too large for one launch", -1);
  topk_decode_kernel<<<dim3((unsigned)bx, (unsigned)nclients), 256, 0, (hipStream_t)stream>>>(
      (const uint8_t*)image, chunk_stride, S, first, first_step, (const f16*)g16, n16, g32, n16 + n32, layout, k, out,
      out_stride);
  MF_CHECK_LAUNCH();
  return 0;
}
