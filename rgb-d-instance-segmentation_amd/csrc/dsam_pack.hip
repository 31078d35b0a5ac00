// K5 weight packing: the float32 segment-form B operand (k_pack_dsam), the bf16 code-merged
// filters of the codes present (k_pack_codes) and the code-presence masks that select them
// (k_code_masks), with their C entry points.
#include "dsam_common.hpp"

using namespace rgbd;
using namespace rgbd::k5;

namespace {

template <typename T>
__global__ void k_pack_dsam(const float* __restrict__ conv_w, const float* __restrict__ proj_w, int Cin,
                            int Cout, T* __restrict__ wfwd, T* __restrict__ wbwd) {
  // element (seg, o, c, tap) of W_seg
  const long long total = 5ll * Cout * Cin * 9;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int tap = (int)(e % 9);
    const int c = (int)((e / 9) % Cin);
    const int o = (int)((e / (9ll * Cin)) % Cout);
    const int seg = (int)(e / (9ll * Cin * Cout));
    const float v = seg < 4 ? conv_w[(((long long)seg * Cout + o) * Cin + c) * 9 + tap]
                            : proj_w[((long long)o * Cin + c) * 9 + tap];
    const T tv = Num<T>::from_f(v);
    if (wfwd) wfwd[(long long)o * 45 * Cin + ((long long)seg * 9 + tap) * Cin + c] = tv;
    if (wbwd) wbwd[(long long)c * 45 * Cout + ((long long)seg * 9 + tap) * Cout + o] = tv;
  }
}

// bf16 code-merged filters W_k = proj + sum_{i in k} conv_i (fixed summation order: proj, then
// conv_0..conv_3, in f32, rounded once), packed for the codes present in the batch only (bit k of
// *code_mask; all 16 when code_mask is NULL), as the B tiles of k_dsam_lds:
//   wfwd [16 code][9 tap][Cin/32 chunk][Cout n][32 c]   (forward: rows n = output channels)
//   wbwd [16 code][9 tap][Cout/32 chunk][Cin n][32 o]   (dX: rows n = input channels)
// so the tile of one (code, tap, chunk) is contiguous (one linear LDS-DMA stream), with the four
// 16-byte chunks of each 64-byte row stored XOR-swizzled by lds_swz(n) (the LDS image the MFMA
// fragment reads want; dsam_common.hpp).  A one-tile tail pad keeps an over-reading last N tile in
// bounds.
//
// Both packings from one pass over the f32 weights.  Workgroup = a block of PK_OB output x PK_CB
// input channels: its 5 x PK_OB rows of (32 c x 9 taps) f32 (conv_0..3, proj; 1152 contiguous
// bytes each in OIHW) are staged in LDS by 16-byte loads, all in flight together.  A unit is 8
// consecutive channels of one (row, tap): wfwd units (o, tap, 8 c) and wbwd units (c, tap, 8 o);
// each reads its 5 x 8 segment values once and writes one 16-byte chunk per present code.  Rows
// are padded to 289 floats so the unit reads of a wave fall on distinct banks.
constexpr int PK_OB = 16, PK_CB = 32, PK_LD = PK_CB * 9 + 1;
constexpr size_t PK_SMEM = 5 * PK_OB * PK_LD * sizeof(float);
__global__ __launch_bounds__(256) void k_pack_codes(const float* __restrict__ conv_w, const float* __restrict__ proj_w,
                                                    int Cin, int Cout, const uint32_t* __restrict__ code_mask,
                                                    bf16_t* __restrict__ wfwd, bf16_t* __restrict__ wbwd) {
  extern __shared__ float sw[];  // [5 seg][PK_OB o][PK_LD]: element (o, c, tap) at c * 9 + tap
  const int c0 = blockIdx.x * PK_CB, o0 = blockIdx.y * PK_OB, tid = threadIdx.x;
  const int nci = Cin / 32, nco = Cout / 32;
  if (blockIdx.x == 0 && blockIdx.y == 0)  // tail pads (read only by an over-reaching last N tile)
    for (int i = tid; i < 192 * 32; i += 256) {
      wfwd[144ll * Cin * Cout + i] = 0;
      if (wbwd) wbwd[144ll * Cin * Cout + i] = 0;
    }
  constexpr int NQ = 5 * PK_OB * (PK_CB * 9 / 4);  // float4 pieces of the block
  constexpr int PER = (NQ + 255) / 256;
  float4 v[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + 256 * j;
    if (i < NQ) {
      const int row = i / (PK_CB * 9 / 4), q = i - row * (PK_CB * 9 / 4), seg = row / PK_OB, o = o0 + row % PK_OB;
      const float* src = seg < 4 ? conv_w + (((long long)seg * Cout + o) * Cin + c0) * 9 : proj_w + ((long long)o * Cin + c0) * 9;
      v[j] = reinterpret_cast<const float4*>(src)[q];
    }
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + 256 * j;
    if (i < NQ) {
      const int row = i / (PK_CB * 9 / 4), q = i - row * (PK_CB * 9 / 4);
      float* d = sw + row * PK_LD + 4 * q;
      d[0] = v[j].x;
      d[1] = v[j].y;
      d[2] = v[j].z;
      d[3] = v[j].w;
    }
  }
  __syncthreads();
  const uint32_t m = code_mask ? *code_mask : 0xffffu;
  // units 0..575: wfwd (tap, o, 8-c chunk q); 576..1151: wbwd (tap, c, 8-o chunk q)
  const int nunits = wbwd ? 2 * 9 * PK_OB * 4 : 9 * PK_OB * 4;
  for (int u = tid; u < nunits; u += 256) {
    const bool bwd = u >= 9 * PK_OB * 4;
    const int w = bwd ? u - 9 * PK_OB * 4 : u;
    const int tap = w / (PK_OB * 4);
    int base, step;  // LDS offset of value e: base + e * step (+ seg * PK_OB * PK_LD)
    long long dst0;  // element offset of the unit's 16-byte chunk for code 0
    long long kstride;
    if (!bwd) {
      const int ol = (w >> 2) & (PK_OB - 1), q = w & 3, n = o0 + ol;
      base = ol * PK_LD + 8 * q * 9 + tap;
      step = 9;
      dst0 = (((long long)tap * nci + blockIdx.x) * Cout + n) * 32 + 8 * ((q ^ lds_swz(n)) & 3);
      kstride = 9ll * nci * Cout * 32;
    } else {
      const int cl = (w >> 1) & (PK_CB - 1), q = w & 1, n = c0 + cl, qo = (o0 & 31) / 8 + q;
      base = 8 * q * PK_LD + cl * 9 + tap;
      step = PK_LD;
      dst0 = (((long long)tap * nco + (o0 >> 5)) * Cin + n) * 32 + 8 * ((qo ^ lds_swz(n)) & 3);
      kstride = 9ll * nco * Cin * 32;
    }
    float s[5][8];
#pragma unroll
    for (int sg = 0; sg < 5; ++sg)
#pragma unroll
      for (int e = 0; e < 8; ++e) s[sg][e] = sw[sg * PK_OB * PK_LD + base + e * step];
    bf16_t* out = bwd ? wbwd : wfwd;
    for (int k = 0; k < 16; ++k) {
      if (!((m >> k) & 1u)) continue;
      float r[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = s[4][e];  // proj, then conv_0..conv_3 of the code's bits, in f32, rounded once
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((k >> i) & 1) t += s[i][e];
        r[e] = t;
      }
      *reinterpret_cast<uint4*>(out + dst0 + k * kstride) =
          make_uint4(pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7]));
    }
  }
}

// OR of (1 << code) over each code map (codes present per DSAM input resolution).
struct CodeMaps {
  const uint8_t* p[8];
  long long n[8];
};
__global__ __launch_bounds__(256) void k_code_masks(CodeMaps cm, uint32_t* __restrict__ masks) {
  const int y = blockIdx.y;
  const uint8_t* p = cm.p[y];
  const long long n = cm.n[y];
  uint32_t m = 0u;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) m |= 1u << (p[i] & 15);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m |= (uint32_t)__shfl_xor((int)m, o);
  if ((threadIdx.x & 63) == 0 && m) atomicOr(masks + y, m);
}

}  // namespace

extern "C" {

long long rgbd_dsam_packed_elems(int dtype, int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0) return 0;
  if (dtype == RGBD_F32) return 45ll * Cin * Cout;
  if (dtype == RGBD_BF16) return 144ll * Cin * Cout + 192 * 32;  // + one-tile tail pad
  return 0;
}

int rgbd_dsam_code_masks(int n, const uint8_t* const* codes_host, const long long* nbytes_host, uint32_t* masks,
                         void* stream) {
  RGBD_REQUIRE(n > 0 && n <= 8 && codes_host && nbytes_host && masks, RGBD_E_ARG);
  CodeMaps cm = {};
  long long most = 1;
  for (int i = 0; i < n; ++i) {
    RGBD_REQUIRE(codes_host[i] && nbytes_host[i] > 0, RGBD_E_ARG);
    cm.p[i] = codes_host[i];
    cm.n[i] = nbytes_host[i];
    most = std::max(most, nbytes_host[i]);
  }
  hipStream_t s = (hipStream_t)stream;
  const hipError_t me = hipMemsetAsync(masks, 0, sizeof(uint32_t) * n, s);
  if (me != hipSuccess) return (int)me;
  k_code_masks<<<dim3((unsigned)std::min<long long>(ceil_div(most, 256 * 8), 256), n), 256, 0, s>>>(cm, masks);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_dsam_pack_weights(int dtype, const float* conv_w, const float* proj_w, int Cin, int Cout,
                           const uint32_t* code_mask, void* wfwd, void* wbwd, void* stream) {
  RGBD_REQUIRE(conv_w && proj_w && (wfwd || wbwd) && Cin > 0 && Cout > 0, RGBD_E_ARG);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_F32) {
    const int nb = (int)std::min<long long>(ceil_div(45ll * Cin * Cout, 256), 4096);
    k_pack_dsam<float><<<nb, 256, 0, s>>>(conv_w, proj_w, Cin, Cout, (float*)wfwd, (float*)wbwd);
  } else if (dtype == RGBD_BF16) {
    RGBD_REQUIRE(wfwd, RGBD_E_ARG);  // wbwd is the transpose of wfwd
    RGBD_REQUIRE(Cin % PK_CB == 0 && Cout % 32 == 0, RGBD_E_SHAPE);
    static const hipError_t attr = hipFuncSetAttribute((const void*)k_pack_codes,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)PK_SMEM);
    if (attr != hipSuccess) return (int)attr;
    k_pack_codes<<<dim3(Cin / PK_CB, Cout / PK_OB), 256, PK_SMEM, s>>>(conv_w, proj_w, Cin, Cout, code_mask,
                                                                       (bf16_t*)wfwd, (bf16_t*)wbwd);
  } else {
    return RGBD_E_DTYPE;
  }
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
