// coarse_half_level.hip -- see coarse_half.h.  The kernels are the three intermediate-level products of coarse_op.hip
// (coarse_apply_once_kernel + its finish pass, coarse_site_kernel in its full and hopping-term forms, coarse_block_minres_kernel)
// on the 16-bit copy: the same workgroup shapes, the same LDS plans, every matrix streamed in 16-byte loads per lane, converted
// in registers and accumulated in fp32.
#include "coarse_half.h"
#include "coarse_half_device.h"

namespace ddamg {

enum { HALF_LEVEL_FULL = 0, HALF_LEVEL_HOP = 1 };   // template argument of coarse_half_site_kernel, as MODE_FULL / MODE_HOP of coarse_site_kernel

// one wavefront, one link L streamed once: res_fwd = s L vj (the term of the link's owner) and res_bwd = s G5 L^H G5 vi (the
// term of its +mu neighbour): wave_mv2 of coarse_op.hip on the 16-bit copy
template <int NT>
__device__ __forceinline__ void wave_mv2_half(const __half2* __restrict__ Mbase, float s, const float* __restrict__ vj, const float* __restrict__ vi, int n,
                                              float* __restrict__ res_fwd, float* __restrict__ res_bwd) {
  const int l = threadIdx.x & 63, a = l >> 3, b = l & 7;
  const int half = n >> 1;
  float xr[NT], xi[NT], wr[NT], wi[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int k = b + 8 * t, kc = k < n ? k : n - 1;   // unconditional loads, see wave_mv_half
    const float2 zj = *reinterpret_cast<const float2*>(vj + 2 * kc);
    xr[t] = k < n ? zj.x : 0.f; xi[t] = k < n ? zj.y : 0.f;
    const int k2 = a + 8 * t, k2c = k2 < n ? k2 : n - 1;
    const float2 zi = *reinterpret_cast<const float2*>(vi + 2 * k2c);
    const float sg = k2 >= n ? 0.f : k2 >= half ? -1.f : 1.f;
    wr[t] = sg * zi.x; wi[t] = sg * zi.y;
  }
  float ar[NT], ai[NT], br[NT], bi[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) { ar[t] = 0; ai[t] = 0; br[t] = 0; bi[t] = 0; }
  const auto fma_tile = [&](int p, int q, const __half2 h) {
    // every product as one fma whose matrix operand is the fp16 number itself (v_fma_mix_f32): no converted copy of the tile
    // group in registers, which the resident self couplings of the block solver need
    const float mr = __low2float(h), mi = __high2float(h);
    ar[p] = fmaf(mr, xr[q], fmaf(-mi, xi[q], ar[p]));
    ai[p] = fmaf(mr, xi[q], fmaf(mi, xr[q], ai[p]));
    br[q] = fmaf(mr, wr[p], fmaf(mi, wi[p], br[q]));
    bi[q] = fmaf(mr, wi[p], fmaf(-mi, wr[p], bi[q]));
  };
  constexpr int TILES = NT * NT, GROUPS = TILES / 4;
  const Half2x4* M4 = reinterpret_cast<const Half2x4*>(Mbase) + l;
#pragma unroll
  for (int g = 0; g < GROUPS; g++) {
    const Half2x4 w = M4[g * 64];
#pragma unroll
    for (int u = 0; u < 4; u++) fma_tile((4 * g + u) / NT, (4 * g + u) % NT, w.e[u]);
  }
  if constexpr (TILES % 4 != 0) fma_tile(NT - 1, NT - 1, Mbase[(TILES - 1) * 64 + l]);   // nt odd: the one tile outside the groups
#pragma unroll
  for (int t = 0; t < NT; t++) {
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) { ar[t] += __shfl_xor(ar[t], o, 64); ai[t] += __shfl_xor(ai[t], o, 64); }
    if (b == 0) { res_fwd[2 * (a + 8 * t)] = s * ar[t]; res_fwd[2 * (a + 8 * t) + 1] = s * ai[t]; }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) { br[t] += __shfl_xor(br[t], o, 64); bi[t] += __shfl_xor(bi[t], o, 64); }
    if (a == 0) {
      const int k = b + 8 * t;
      const float sg = (k >= half) ? -s : s;
      res_bwd[2 * k] = sg * br[t]; res_bwd[2 * k + 1] = sg * bi[t];
    }
  }
}

// a matrix of the copy in registers: lane l holds its four elements of every tile group, and element l of the tail tile
template <int NT>
struct HalfTiles {
  static constexpr int TILES = NT * NT, GROUPS = TILES / 4;
  Half2x4 g[GROUPS > 0 ? GROUPS : 1];
  __half2 tail;
  __device__ __forceinline__ void load(const __half2* __restrict__ Mbase, int l) {
    const Half2x4* M4 = reinterpret_cast<const Half2x4*>(Mbase) + l;
#pragma unroll
    for (int k = 0; k < GROUPS; k++) g[k] = M4[k * 64];
    if constexpr (TILES % 4 != 0) tail = Mbase[(TILES - 1) * 64 + l];
  }
};

// res = s * M v with the matrix already in registers: self couplings that a wavefront applies in every MinRes step of a block
template <int NT>
__device__ __forceinline__ void wave_mv_reg_half(const HalfTiles<NT>& m, float s, const float* __restrict__ v, int n, float* __restrict__ res) {
  const int l = threadIdx.x & 63, a = l >> 3, b = l & 7;
  float xr[NT], xi[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int k = b + 8 * t, kc = k < n ? k : n - 1;
    const float2 z = *reinterpret_cast<const float2*>(v + 2 * kc);
    xr[t] = k < n ? z.x : 0.f; xi[t] = k < n ? z.y : 0.f;
  }
  float ar[NT], ai[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) { ar[t] = 0; ai[t] = 0; }
  const auto fma_tile = [&](int p, int q, const __half2 h) {
    const float mr = __low2float(h), mi = __high2float(h);   // see wave_mv2_half
    ar[p] = fmaf(mr, xr[q], fmaf(-mi, xi[q], ar[p]));
    ai[p] = fmaf(mr, xi[q], fmaf(mi, xr[q], ai[p]));
  };
#pragma unroll
  for (int g = 0; g < HalfTiles<NT>::GROUPS; g++)
#pragma unroll
    for (int u = 0; u < 4; u++) fma_tile((4 * g + u) / NT, (4 * g + u) % NT, m.g[g].e[u]);
  if constexpr (HalfTiles<NT>::TILES % 4 != 0) fma_tile(NT - 1, NT - 1, m.tail);
#pragma unroll
  for (int t = 0; t < NT; t++) {
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) { ar[t] += __shfl_xor(ar[t], o, 64); ai[t] += __shfl_xor(ai[t], o, 64); }
    if (b == 0) { res[2 * (a + 8 * t)] = s * ar[t]; res[2 * (a + 8 * t) + 1] = s * ai[t]; }
  }
}

// ---- listed / masked site kernel: coarse_site_kernel<float, NT, MODE_FULL | MODE_HOP> on the copy --------------------------
//   out(x) = [accumulate ? out(x) : 0] + sign_self * M0 in(x) + sign_hop * sum_{d in mask(x)} hop_d(in),  x = site_list[bid] or s0 + bid
// HALF_LEVEL_FULL: wavefront 0 the self coupling, 1-4 the forward links of x, 5-8 the backward couplings from the forward links
// of the neighbours; HALF_LEVEL_HOP: the eight hopping terms only.  The neighbour table holds sites only: the copy is not
// made for a level that is decomposed over processes.
template <int NT, int mode>
__global__ __launch_bounds__(mode == HALF_LEVEL_FULL ? 576 : 512) void coarse_half_site_kernel(float* __restrict__ out, const float* __restrict__ in, CoarseHalfDev op, int s0,
                                                                                              float sign_self, float sign_hop, int accumulate,
                                                                                              const int* __restrict__ site_list, const unsigned char* __restrict__ dir_mask,
                                                                                              int mask_invert, int swizzle) {
  constexpr int np = 8 * NT, NW = mode == HALF_LEVEL_FULL ? 9 : 8;
  __shared__ float res[NW * 2 * np];
  int bid = blockIdx.x;
  if (swizzle) {   // the XCD swizzle of coarse_site_kernel
    const int chunk = gridDim.x >> 3;
    if (bid < chunk * 8) bid = (bid & 7) * chunk + (bid >> 3);
  }
  const int x = site_list ? site_list[bid] : s0 + bid;
  // directions (bit d: +T,+Z,+Y,+X,-T,-Z,-Y,-X) whose hopping term is included for this site
  unsigned dmask = 0xffu;
  if (dir_mask) dmask = mask_invert ? (~(unsigned)dir_mask[x]) & 0xffu : (unsigned)dir_mask[x];
  const int w = threadIdx.x >> 6;
  const int n = op.n;
  const size_t V = op.V;
  float* r = res + (size_t)w * 2 * np;
  const int prod = mode == HALF_LEVEL_HOP ? w + 1 : w;   // 0 self, 1..4 fwd, 5..8 bwd
  if (prod == 0) {
    wave_mv_half<NT, false>(op.M + (size_t)x * 5 * op.msize, op.scale[(size_t)x * 6], in + (size_t)x * n * 2, n, r);
  } else if (!((dmask >> (prod - 1)) & 1u)) {
    for (int k = threadIdx.x & 63; k < 2 * np; k += 64) r[k] = 0;   // direction masked out
  } else if (prod <= 4) {
    const int mu = prod - 1;
    const int y = op.nb[(size_t)mu * V + x];
    wave_mv_half<NT, false>(op.M + ((size_t)x * 5 + 1 + mu) * op.msize, op.scale[(size_t)x * 6 + 1 + mu], in + (size_t)y * n * 2, n, r);
  } else {
    const int mu = prod - 5;
    const int y = op.nb[(size_t)(4 + mu) * V + x];
    wave_mv_half<NT, true>(op.M + ((size_t)y * 5 + 1 + mu) * op.msize, op.scale[(size_t)y * 6 + 1 + mu], in + (size_t)y * n * 2, n, r);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * n; k += blockDim.x) {
    float v = accumulate ? out[(size_t)x * n * 2 + k] : 0.f;
    if (mode == HALF_LEVEL_FULL) {
      v += sign_self * res[k];
      for (int ww = 1; ww < NW; ww++) v += sign_hop * res[(size_t)ww * 2 * np + k];
    } else {
      float s = 0;
      for (int ww = 0; ww < NW; ww++) s += res[(size_t)ww * 2 * np + k];
      v += sign_hop * s;
    }
    out[(size_t)x * n * 2 + k] = v;
  }
}

// ---- full operator with every link read once: coarse_apply_once_kernel<float, NT, false> + its finish pass on the copy -----
// Phase 1, one workgroup per site x: wavefront 0 the self coupling, wavefronts 1-4 one forward link each -- L in(x+mu) for x
// itself and G5 L^H G5 in(x), the backward term of x+mu, which goes to bwd[mu][x+mu].  Phase 2: out(x) -= sum_mu bwd[mu][x].
template <int NT>
__global__ __launch_bounds__(320) void coarse_half_apply_once_kernel(float* __restrict__ out, float* __restrict__ bwd, const float* __restrict__ in, CoarseHalfDev op) {
  constexpr int np = 8 * NT;
  __shared__ float res[5 * 2 * np];
  __shared__ float tmpb[4 * 2 * np];
  int bid = blockIdx.x;
  { const int chunk = gridDim.x >> 3; if (bid < chunk * 8) bid = (bid & 7) * chunk + (bid >> 3); }
  const int x = bid, w = threadIdx.x >> 6, n = op.n;
  const size_t V = op.V;
  int y = -1;
  if (w == 0) {
    wave_mv_half<NT, false>(op.M + (size_t)x * 5 * op.msize, op.scale[(size_t)x * 6], in + (size_t)x * n * 2, n, res);
  } else {
    const int mu = w - 1;
    y = op.nb[(size_t)mu * V + x];
    wave_mv2_half<NT>(op.M + ((size_t)x * 5 + 1 + mu) * op.msize, op.scale[(size_t)x * 6 + 1 + mu], in + (size_t)y * n * 2, in + (size_t)x * n * 2, n,
                      res + (size_t)w * 2 * np, tmpb + (size_t)mu * 2 * np);
  }
  __syncthreads();
  if (w > 0) {
    const int mu = w - 1;
    float* dst = bwd + ((size_t)mu * V + y) * n * 2;
    for (int k = threadIdx.x & 63; k < 2 * n; k += 64) dst[k] = tmpb[(size_t)mu * 2 * np + k];
  }
  for (int k = threadIdx.x; k < 2 * n; k += blockDim.x)
    out[(size_t)x * n * 2 + k] = res[k] - (res[2 * np + k] + res[4 * np + k] + res[6 * np + k] + res[8 * np + k]);
}
__global__ __launch_bounds__(256) void coarse_half_apply_once_finish_kernel(float* __restrict__ out, const float* __restrict__ bwd, size_t V, size_t n2) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * n2) return;
  float s = 0;
#pragma unroll
  for (int mu = 0; mu < 4; mu++) s += bwd[(size_t)mu * V * n2 + i];
  out[i] -= s;
}

// ---- fused block solver: coarse_block_minres_kernel<float, NT> on the copy -------------------------------------------------
// Items, contrib plan, LDS vectors in fp32, fp64 block sums and the eps guard as there.  Self couplings stay in registers across
// the MinRes steps (NT * NT VGPRs each, half of what fp32 needs), two per wavefront where the register budget of 8 wavefronts
// per workgroup allows it: every self coupling of a 16-site block is resident then and a step streams the block's links only
// (32 instead of 48 matrices for a 2^4 block).  At NT = 6 two per wavefront spill (160 bytes of scratch per lane in the
// compiler's report): one there, as in fp32.
constexpr int HALF_MINRES_THREADS = 512, HALF_MINRES_MAXE = 4;
template <int NT>
__global__ __launch_bounds__(HALF_MINRES_THREADS) void coarse_half_block_minres_kernel(float* __restrict__ x, float* __restrict__ r, float* __restrict__ latest, CoarseHalfDev op,
                                                                                       const int* __restrict__ blocks, const int* __restrict__ items, int nitems,
                                                                                       const int* __restrict__ contrib, int BS, int iters, double eps) {
  extern __shared__ double smem_d[];
  constexpr int np = 8 * NT, NTH = HALF_MINRES_THREADS;
  double* red = smem_d;                                       // [3][16]
  float* rl = reinterpret_cast<float*>(smem_d + 48);          // [BS][2 np]
  float* lphi = rl + (size_t)BS * 2 * np;                     // [BS][2 np]
  float* slots = lphi + (size_t)BS * 2 * np;                  // [2 nitems][2 np]
  const int n = op.n, tid = threadIdx.x, w = tid >> 6, nw = NTH >> 6;
  const size_t s0 = (size_t)blocks[blockIdx.x] * BS;
  for (int e = tid; e < BS * 2 * np; e += NTH) {
    const int i = e / (2 * np), k = e - i * 2 * np;
    rl[e] = k < 2 * n ? r[(s0 + i) * n * 2 + k] : 0.f;
    lphi[e] = 0;
  }
  constexpr int ITEMS_MAX = 128;   // the item table in LDS (coarse_block_minres_kernel)
  __shared__ int sitems[3 * ITEMS_MAX];
  const bool items_in_lds = nitems <= ITEMS_MAX;
  if (items_in_lds) for (int e = tid; e < 3 * nitems; e += NTH) sitems[e] = items[e];
  const int* __restrict__ itab = items_in_lds ? sitems : items;
  __syncthreads();
  // the first BS items are the self couplings: wavefront w keeps those of the sites w, w + nw, ... below nres, everything from
  // item nres on is streamed
  constexpr int RES = NT <= 5 ? 2 : 1;
  constexpr bool resident = NT <= 6;
  const int nres = resident ? (BS < RES * nw ? BS : RES * nw) : 0;
  HalfTiles<NT> mres[RES];
  float sres[RES];
  if (resident) {
#pragma unroll
    for (int q = 0; q < RES; q++) {
      const int item = w + q * nw;
      if (item < nres) {
        mres[q].load(op.M + (s0 + item) * 5 * op.msize, tid & 63);
        sres[q] = op.scale[(s0 + item) * 6];
      }
    }
  }
  for (int it = 0; it < iters; it++) {
    if (resident) {
#pragma unroll
      for (int q = 0; q < RES; q++) {
        const int item = w + q * nw;      // self items are (i, -1, i) with i = item
        if (item < nres) wave_mv_reg_half<NT>(mres[q], sres[q], rl + (size_t)item * 2 * np, n, slots + (size_t)(2 * item) * 2 * np);
      }
    }
    for (int item = nres + w; item < nitems; item += nw) {
      const int i = itab[3 * item], mu = itab[3 * item + 1], j = itab[3 * item + 2];
      const __half2* Mx = op.M + (s0 + i) * 5 * op.msize;
      const float* sx = op.scale + (s0 + i) * 6;
      if (mu < 0) wave_mv_half<NT, false>(Mx, sx[0], rl + (size_t)i * 2 * np, n, slots + (size_t)(2 * item) * 2 * np);
      else wave_mv2_half<NT>(Mx + (size_t)(1 + mu) * op.msize, sx[1 + mu], rl + (size_t)j * 2 * np, rl + (size_t)i * 2 * np, n,
                             slots + (size_t)(2 * item) * 2 * np, slots + (size_t)(2 * item + 1) * 2 * np);
    }
    __syncthreads();
    double s[3] = {0, 0, 0};
    float dre[HALF_MINRES_MAXE], dim[HALF_MINRES_MAXE];
#pragma unroll
    for (int u = 0; u < HALF_MINRES_MAXE; u++) {
      const int c = tid + u * NTH;
      dre[u] = 0; dim[u] = 0;
      if (c < BS * n) {
        const int i = c / n, k = c - i * n;
        const int* ct = contrib + i * 10;
        const int cnt = ct[0];
        float dr = slots[(size_t)ct[1] * 2 * np + 2 * k], di = slots[(size_t)ct[1] * 2 * np + 2 * k + 1];
        for (int q = 2; q <= cnt; q++) { dr -= slots[(size_t)ct[q] * 2 * np + 2 * k]; di -= slots[(size_t)ct[q] * 2 * np + 2 * k + 1]; }
        const double rr = rl[(size_t)i * 2 * np + 2 * k], ri = rl[(size_t)i * 2 * np + 2 * k + 1];
        s[0] += (double)dr * rr + (double)di * ri; s[1] += (double)dr * ri - (double)di * rr; s[2] += (double)dr * dr + (double)di * di;
        dre[u] = dr; dim[u] = di;
      }
    }
    // block sum (every thread gets it; the barrier lets the slots be overwritten afterwards)
    {
      const int lane = tid & 63;
#pragma unroll
      for (int k = 0; k < 3; k++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
      if (lane == 0) { red[w] = s[0]; red[16 + w] = s[1]; red[32 + w] = s[2]; }
      __syncthreads();
      s[0] = 0; s[1] = 0; s[2] = 0;
      for (int ww = 0; ww < nw; ww++) { s[0] += red[ww]; s[1] += red[16 + ww]; s[2] += red[32 + ww]; }
    }
    float ar = 0, ai = 0;
    if (fabs(s[2]) >= eps) { ar = (float)(s[0] / s[2]); ai = (float)(s[1] / s[2]); }
#pragma unroll
    for (int u = 0; u < HALF_MINRES_MAXE; u++) {
      const int c = tid + u * NTH;
      if (c < BS * n) {
        const int i = c / n, k = c - i * n;
        const size_t o = (size_t)i * 2 * np + 2 * k;
        const float rr = rl[o], ri = rl[o + 1];
        lphi[o] += ar * rr - ai * ri; lphi[o + 1] += ar * ri + ai * rr;
        rl[o] = rr - (ar * dre[u] - ai * dim[u]); rl[o + 1] = ri - (ar * dim[u] + ai * dre[u]);
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < BS * 2 * n; e += NTH) {
    const int i = e / (2 * n), k = e - i * 2 * n;
    const size_t g = (s0 + i) * n * 2 + k;
    const float d = lphi[(size_t)i * 2 * np + k];
    r[g] = rl[(size_t)i * 2 * np + k];
    latest[g] = d;
    x[g] += d;
  }
}

// ---- host side: CoarseHalf's three products of an intermediate level (refresh and release: coarse_half.hip) ------------------
static void launch_half_site(const CoarseHalfDev& h, int nt, float* out, const float* in, int nsites, bool full, double ss, double sh, bool acc,
                             const int* site_list, const unsigned char* dir_mask, bool mask_invert, hipStream_t st) {
  if (nsites <= 0) return;
  DDAMG_REQUIRE(nsites <= h.V, "16-bit intermediate storage: more sites than the level has");
  const dim3 grid(nsites), block(full ? 576 : 512);
  const int swz = nsites >= 64 ? 1 : 0;
#define DDAMG_LAUNCH(NTV, MODEV) hipLaunchKernelGGL((coarse_half_site_kernel<NTV, MODEV>), grid, block, 0, st, out, in, h, 0, (float)ss, (float)sh, acc ? 1 : 0, \
                                                    site_list, dir_mask, mask_invert ? 1 : 0, swz)
#define DDAMG_CASE(NTV) case NTV: if (full) DDAMG_LAUNCH(NTV, HALF_LEVEL_FULL); else DDAMG_LAUNCH(NTV, HALF_LEVEL_HOP); break;
  switch (nt) {
    DDAMG_CASE(1) DDAMG_CASE(2) DDAMG_CASE(3) DDAMG_CASE(4) DDAMG_CASE(5) DDAMG_CASE(6) DDAMG_CASE(7) DDAMG_CASE(8)
    default: DDAMG_REQUIRE(false, "coarse operator: more than 64 dof per site are not supported");
  }
#undef DDAMG_CASE
#undef DDAMG_LAUNCH
  DDAMG_HIP_CHECK(hipGetLastError());
}

void CoarseHalf::apply(const CoarseOp<float>& op, float* out, const float* in, hipStream_t st) {
  DDAMG_REQUIRE(out != in, "coarse apply cannot run in place");
  const CoarseHalfDev h = refresh(op, st, false);
  if (op.V() < op.knobs().coarse_apply_once_min_sites) {   // the threshold of CoarseOp::apply
    launch_half_site(h, op.nt(), out, in, op.V(), true, 1.0, -1.0, false, nullptr, nullptr, false, st);
    return;
  }
  float* bwd = op.backward_workspace();
#define DDAMG_CASE(NTV) case NTV: hipLaunchKernelGGL((coarse_half_apply_once_kernel<NTV>), dim3(op.V()), dim3(320), 0, st, out, bwd, in, h); break;
  switch (op.nt()) {
    DDAMG_CASE(1) DDAMG_CASE(2) DDAMG_CASE(3) DDAMG_CASE(4) DDAMG_CASE(5) DDAMG_CASE(6) DDAMG_CASE(7) DDAMG_CASE(8)
    default: DDAMG_REQUIRE(false, "coarse operator: more than 64 dof per site are not supported");
  }
#undef DDAMG_CASE
  const size_t V = (size_t)op.V(), n2 = (size_t)op.n() * 2;
  hipLaunchKernelGGL(coarse_half_apply_once_finish_kernel, dim3((unsigned)((V * n2 + 255) / 256)), dim3(256), 0, st, out, bwd, V, n2);
  DDAMG_HIP_CHECK(hipGetLastError());
}

void CoarseHalf::apply_masked(const CoarseOp<float>& op, float* out, const float* in, const int* site_list, int nsites, const unsigned char* dir_mask,
                                   bool mask_invert, double sign_self, double sign_hop, bool accumulate, hipStream_t st) {
  DDAMG_REQUIRE(out != in, "coarse apply cannot run in place");
  const CoarseHalfDev h = refresh(op, st, false);
  launch_half_site(h, op.nt(), out, in, nsites, sign_self != 0.0, sign_self, sign_hop, accumulate, site_list, dir_mask, mask_invert, st);
}

bool CoarseHalf::block_minres(const CoarseOp<float>& op, float* x, float* r, float* latest, const int* blocks, int nblocks,
                                   const CoarseOp<float>::BlockPlan& plan, int iters, double eps, hipStream_t st) {
  // the shape limits of CoarseOp::block_minres
  const int np = 8 * op.nt(), BS = plan.block_sites;
  const size_t lds = 48 * sizeof(double) + sizeof(float) * 2 * np * ((size_t)2 * BS + (size_t)2 * plan.nitems);
  if (op.knobs().coarse_sap_unfused || plan.nitems == 0 || (size_t)BS * op.n() > (size_t)HALF_MINRES_THREADS * HALF_MINRES_MAXE || lds > 150 * 1024) return false;
  if (nblocks <= 0) return true;
  const CoarseHalfDev h = refresh(op, st, false);
#define DDAMG_CASE(NTV) case NTV: \
    DDAMG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&coarse_half_block_minres_kernel<NTV>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL((coarse_half_block_minres_kernel<NTV>), dim3(nblocks), dim3(HALF_MINRES_THREADS), lds, st, x, r, latest, h, blocks, plan.d_items, plan.nitems, \
                       plan.d_contrib, BS, iters, eps); break;
  switch (op.nt()) {
    DDAMG_CASE(1) DDAMG_CASE(2) DDAMG_CASE(3) DDAMG_CASE(4) DDAMG_CASE(5) DDAMG_CASE(6) DDAMG_CASE(7) DDAMG_CASE(8)
    default: return false;
  }
#undef DDAMG_CASE
  DDAMG_HIP_CHECK(hipGetLastError());
  return true;
}

}  // namespace ddamg
