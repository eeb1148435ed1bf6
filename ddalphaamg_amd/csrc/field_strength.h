// field_strength.h -- the bodies of the kernels that take the operator fields from links the caller keeps in device memory
// (gauge_device.hip: field_strength_kernel, clover_assemble_kernel).  Reference: Q / Qdiff / set_clover src/dirac.c:304-402,
// calc_plaq :568-622.
//
// One workgroup = one wave = an 8 x 8 tile of sites of ONE plane (mu, nu), mu < nu.  The four leaves of Q_{mu nu} at the sites
// of the tile read U_mu on (8+1) x (8+2) and U_nu on (8+2) x (8+1) sites of the plane and no other link, so the workgroup
// stages the (8+2) x (8+2) neighbourhood of both directions in LDS once (200 links for 128 of its own: every link leaves
// memory 1.6 times per plane it lies in, three planes each) and all twelve products of a site read LDS only.
// Q_{nu mu} = Q_{mu nu}^dagger, so the plane's contribution to the clover term is F = (Q - Q^dagger) / 16: anti-Hermitian,
// kept as 9 reals per site and plane.  The plaquette is the trace of the first leaf.
//
// On a process grid the same kernel reads the lattice extended by the neighbours' links (Shell below): the tiles still cover
// own sites only, and only the offsets of the staged neighbourhood differ (stage_offsets<true>).
//
// The bodies are plain functions of (workgroup, thread) so that a host program can run them thread by thread
// (tests/native/link_shell_check.cpp does, for the extended lattice).
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define DDAMG_FS_HD __host__ __device__ __forceinline__
#else
#define DDAMG_FS_HD inline
#endif

namespace ddamg {
namespace fs {

constexpr int TILE = 8;              // sites per direction of the plane tile
constexpr int EXT = TILE + 2;        // with the neighbours one site away
constexpr int NEXT = EXT * EXT;
constexpr int PITCH = 19;            // doubles per staged link: 18 + 1, an odd number of 8-byte bank pairs
constexpr int THREADS = TILE * TILE;
constexpr int LDS_DOUBLES = 2 * NEXT * PITCH;

struct cplx { double r, i; };
struct M3 { cplx a[9]; };

DDAMG_FS_HD M3 mul(const M3& x, const M3& y) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double sr = 0, si = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const cplx a = x.a[3 * i + k], b = y.a[3 * k + j];
        sr += a.r * b.r - a.i * b.i; si += a.r * b.i + a.i * b.r;
      }
      r.a[3 * i + j] = cplx{sr, si};
    }
  return r;
}
DDAMG_FS_HD M3 dag(const M3& x) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) r.a[3 * i + j] = cplx{x.a[3 * j + i].r, -x.a[3 * j + i].i};
  return r;
}

// the six planes mu < nu in the order of the reference's loops, and the two directions outside each
struct Planes {
  int L[4];
  int nblocks[6];   // workgroups of each plane
  int max_blocks;
};
DDAMG_FS_HD int plane_mu(int p) { return p < 3 ? 0 : (p < 5 ? 1 : 2); }
DDAMG_FS_HD int plane_nu(int p) { return p < 3 ? p + 1 : (p < 5 ? p - 1 : 3); }
inline Planes make_planes(const int L[4]) {
  Planes g;
  g.max_blocks = 0;
  size_t V = 1;
  for (int d = 0; d < 4; d++) { g.L[d] = L[d]; V *= (size_t)L[d]; }
  for (int p = 0; p < 6; p++) {
    const int mu = plane_mu(p), nu = plane_nu(p);
    const size_t outside = V / ((size_t)L[mu] * L[nu]);
    const size_t nb = outside * ((L[mu] + TILE - 1) / TILE) * ((L[nu] + TILE - 1) / TILE);
    g.nblocks[p] = (int)nb;
    if (g.nblocks[p] > g.max_blocks) g.max_blocks = g.nblocks[p];
  }
  return g;
}

// where workgroup `block` of plane p sits: the lexicographic offset of the two outside coordinates and the tile origin
struct Tile {
  int mu, nu;
  size_t outside;        // lexicographic site offset of the coordinates outside the plane
  size_t smu, snu;       // site strides of mu and nu
  int a0, b0;            // first mu / nu coordinate of the tile
};
DDAMG_FS_HD Tile tile_of(const Planes& g, int p, int block) {
  Tile t;
  t.mu = plane_mu(p); t.nu = plane_nu(p);
  size_t stride[4];
  stride[3] = 1; stride[2] = (size_t)g.L[3]; stride[1] = stride[2] * g.L[2]; stride[0] = stride[1] * g.L[1];
  t.smu = stride[t.mu]; t.snu = stride[t.nu];
  const int ntb = (g.L[t.nu] + TILE - 1) / TILE, nta = (g.L[t.mu] + TILE - 1) / TILE;
  int r = block;
  t.b0 = (r % ntb) * TILE; r /= ntb;
  t.a0 = (r % nta) * TILE; r /= nta;
  t.outside = 0;
  for (int d = 3; d >= 0; d--)
    if (d != t.mu && d != t.nu) { t.outside += (size_t)(r % g.L[d]) * stride[d]; r /= g.L[d]; }
  return t;
}

// ---- the lattice extended by the neighbours' links on a process grid --------------------------------------------------------
// The own lattice plus a shell `depth` sites deep in every split direction (h[d] = depth; an unsplit direction has h[d] = 0 and
// keeps wrapping periodically inside the process): extents E[d] = L[d] + 2 h[d], own coordinate c in [-h, L + h) stored at c + h,
// lexicographic as the own lattice.  Depth 1 (the leaves of Q, the plaquette staples): the same shell as gauge.cpp builds on the
// host.  Depth 2: the rectangle staples (gauge_md.h).  A split direction needs L[d] >= depth: the shell is cut from ONE neighbour.
struct Shell {
  int L[4], h[4], E[4];
  size_t stride[4];      // site strides of the extended array
  size_t V, Ve;          // own sites, sites of the extended array
};
inline Shell make_shell(const int L[4], const bool split[4], int depth = 1) {
  Shell s;
  s.V = 1; s.Ve = 1;
  for (int d = 0; d < 4; d++) { s.L[d] = L[d]; s.h[d] = split[d] ? depth : 0; s.E[d] = L[d] + 2 * s.h[d]; s.V *= (size_t)L[d]; s.Ve *= (size_t)s.E[d]; }
  s.stride[3] = 1; s.stride[2] = (size_t)s.E[3]; s.stride[1] = s.stride[2] * s.E[2]; s.stride[0] = s.stride[1] * s.E[1];
  return s;
}

// where the own site with lexicographic index lx lies in the extended array; t: its own T coordinate, where asked for
DDAMG_FS_HD size_t extended_site(const Shell& s, size_t lx, int* t = nullptr) {
  size_t r = lx;
  const int x3 = (int)(r % s.L[3]); r /= s.L[3];
  const int x2 = (int)(r % s.L[2]); r /= s.L[2];
  const int x1 = (int)(r % s.L[1]); r /= s.L[1];
  const int x0 = (int)r;
  if (t) *t = x0;
  return (size_t)(x0 + s.h[0]) * s.stride[0] + (size_t)(x1 + s.h[1]) * s.stride[1] + (size_t)(x2 + s.h[2]) * s.stride[2] + (size_t)(x3 + s.h[3]);
}

// W doubles moved by one thread: 2 (one 16-byte access) where every array involved is 16-byte aligned, 1 otherwise
template <int W> struct Reals;
template <> struct alignas(16) Reals<2> { double v[2]; };
template <> struct alignas(8) Reals<1> { double v[1]; };

// links_extend_kernel, thread i of V * 72 / W: W consecutive reals of the caller's links U [V][4][18] into the interior of the
// extended array Ue [Ve][4][18].  negate_last_t != 0: the T-links of the local slice L[0] - 1 change sign on the way (the
// anti-periodic boundary; set on the processes that hold the last global time slice and nowhere else, so that the neighbours
// receive signed links and nobody flips afterwards).  U is read, never written.
template <int W>
DDAMG_FS_HD void extend_links(const Shell& s, const double* __restrict__ U, double* __restrict__ Ue, size_t i, int negate_last_t) {
  constexpr size_t PER_SITE = 72 / W;
  if (i >= s.V * PER_SITE) return;
  const size_t lx = i / PER_SITE; const int k = (int)(i - lx * PER_SITE) * W;   // first real inside the site
  int x0;
  const size_t e = extended_site(s, lx, &x0);
  Reals<W> v = *reinterpret_cast<const Reals<W>*>(U + lx * 72 + k);
  if (negate_last_t && k < 18 && x0 == s.L[0] - 1) {
#pragma unroll
    for (int w = 0; w < W; w++) v.v[w] = -v.v[w];
  }
  *reinterpret_cast<Reals<W>*>(Ue + e * 72 + k) = v;
}

// One slab of the extended array: the h[mu] (the shell's depth) consecutive coordinates of direction mu that start at a given one.
// Directions are exchanged in the order 0, 1, 2, 3; the slab spans the full extended range of the split directions before mu, so
// that what was received there (the corners) travels along, and the own range of the directions after mu.
struct Slab {
  int mu;
  int n[4];          // sites per direction (n[mu] = the depth)
  int first[4];      // stored coordinate of the first one (first[mu]: set by the caller, see slab_at)
  size_t sites;
};
inline Slab make_slab(const Shell& s, int mu) {
  Slab b; b.mu = mu; b.sites = 1;
  for (int d = 0; d < 4; d++) {
    if (d == mu) { b.n[d] = s.h[d]; b.first[d] = 0; }     // an unsplit mu (h = 0) has no slab: sites = 0, and no caller asks for one
    else if (d < mu) { b.n[d] = s.E[d]; b.first[d] = 0; }
    else { b.n[d] = s.L[d]; b.first[d] = s.h[d]; }
    b.sites *= (size_t)b.n[d];
  }
  return b;
}
// the slab whose first own coordinate of direction mu is c: c = L - depth and 0 are packed, -depth and L are filled from what arrived
inline Slab slab_at(const Shell& s, Slab b, int c) { b.first[b.mu] = c + s.h[b.mu]; return b; }

// site `site` of the slab, in the slab's own lexicographic order, as a site of the extended array
DDAMG_FS_HD size_t slab_site(const Shell& s, const Slab& b, size_t site) {
  size_t r = site, e = 0;
#pragma unroll
  for (int d = 3; d >= 0; d--) { e += (size_t)(b.first[d] + (int)(r % b.n[d])) * s.stride[d]; r /= b.n[d]; }
  return e;
}
// link_slab_pack_kernel (to_buffer) / link_slab_unpack_kernel, thread i of sites * 36: 16 bytes, consecutive threads consecutive
// reals of a site; buf [sites][72] in the slab's own lexicographic order, the same on the sender and the receiver
DDAMG_FS_HD void slab_copy(const Shell& s, const Slab& b, double* __restrict__ Ue, double* __restrict__ buf, size_t i, bool to_buffer) {
  if (i >= b.sites * 36) return;
  const size_t site = i / 36; const int k = (int)(i - site * 36) * 2;
  const size_t e = slab_site(s, b, site);
  Reals<2>* in_array = reinterpret_cast<Reals<2>*>(Ue + e * 72 + k);
  Reals<2>* in_buffer = reinterpret_cast<Reals<2>*>(buf + site * 72 + k);
  if (to_buffer) *in_buffer = *in_array; else *in_array = *in_buffer;
}

// where the staged neighbourhood of tile t lies in the extended array: the tile with the extended array's strides and the offset
// of the two outside coordinates there.  Used for the loads only; F and the plaquette keep the own lattice's tile.
DDAMG_FS_HD Tile extended_tile(const Planes& g, const Shell& s, const Tile& t, int block) {
  Tile x = t;
  x.smu = s.stride[t.mu]; x.snu = s.stride[t.nu];
  int r = block / (((g.L[t.nu] + TILE - 1) / TILE) * ((g.L[t.mu] + TILE - 1) / TILE));
  x.outside = 0;
  for (int d = 3; d >= 0; d--)
    if (d != t.mu && d != t.nu) { x.outside += (size_t)(r % g.L[d] + s.h[d]) * s.stride[d]; r /= g.L[d]; }
  return x;
}

// step 1, threads 0 .. 2 EXT - 1: site offset of every mu row (entries 0 .. EXT-1) and nu column (EXT .. 2 EXT - 1) of the
// staged neighbourhood, periodic; flip[i] != 0: the mu links of row i carry the anti-periodic sign (mu = T, last time slice).
// EXTENDED (t: extended_tile, s: its shell): offsets into the extended array.  A split direction is addressed without wrap,
// coordinate c in [-1, L] at c + 1 (rows of a tile tail beyond L, which no site of the lattice reads, stay at L); the others wrap
// as on a single process.  The sign is in the extended array already: nothing is flipped.
template <bool EXTENDED = false>
DDAMG_FS_HD void stage_offsets(const Planes& g, const Tile& t, int anti_pbc, int tid, size_t* off, int* flip, const Shell* s = nullptr) {
  if (tid >= 2 * EXT) return;
  const bool row = tid < EXT;
  const int i = row ? tid : tid - EXT;
  const int Ld = g.L[row ? t.mu : t.nu];
  if constexpr (EXTENDED) {
    const int h = s->h[row ? t.mu : t.nu];
    int c = (row ? t.a0 : t.b0) + i - 1;
    if (h) c = (c > Ld ? Ld : c) + 1;
    else c = (c + Ld) % Ld;
    off[tid] = (size_t)c * (row ? t.smu : t.snu);
    if (row) flip[i] = 0;
  } else {
    const int c = ((row ? t.a0 : t.b0) + i - 1 + Ld) % Ld;
    off[tid] = (size_t)c * (row ? t.smu : t.snu);
    if (row) flip[i] = (anti_pbc && t.mu == 0 && c == g.L[0] - 1) ? 1 : 0;
  }
}

// step 2, all threads: the links of both directions into LDS, lds[(w * NEXT + i * EXT + j) * PITCH + k], w = 0: U_mu, 1: U_nu;
// consecutive threads read consecutive reals of the caller's array
DDAMG_FS_HD void stage_links(const double* __restrict__ U, const Tile& t, int tid, const size_t* off, const int* flip, double* lds) {
  constexpr int TOTAL = 2 * NEXT * 18, BATCH = 8;   // BATCH loads in flight per thread before the first store
  for (int k0 = 0; k0 < TOTAL; k0 += THREADS * BATCH) {
    double v[BATCH]; int dst[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; u++) {
      const int k = k0 + u * THREADS + tid;
      dst[u] = -1; v[u] = 0.0;
      if (k < TOTAL) {
        const int w = k / (NEXT * 18), rem = k - w * (NEXT * 18);
        const int e = rem / 18, comp = rem - e * 18;
        const int i = e / EXT, j = e - i * EXT;
        const size_t lx = t.outside + off[i] + off[EXT + j];
        const double u0 = U[(lx * 4 + (w ? t.nu : t.mu)) * 18 + comp];
        v[u] = (w == 0 && flip[i]) ? -u0 : u0;
        dst[u] = (w * NEXT + e) * PITCH + comp;
      }
    }
#pragma unroll
    for (int u = 0; u < BATCH; u++) if (dst[u] >= 0) lds[dst[u]] = v[u];
  }
}

DDAMG_FS_HD M3 staged(const double* lds, int w, int e) {
  M3 m; const double* p = lds + (w * NEXT + e) * PITCH;
#pragma unroll
  for (int k = 0; k < 9; k++) m.a[k] = cplx{p[2 * k], p[2 * k + 1]};
  return m;
}

// step 3, one thread per site of the tile: F (9 reals: the imaginary parts of the diagonal, then (0,1), (0,2), (1,2)) and the
// real trace of the first leaf.  Returns false for a thread outside the lattice (tile tail).
DDAMG_FS_HD bool site_field_strength(const Planes& g, const Tile& t, int tid, const double* lds, size_t* lex, double (&F)[9], double* plaq) {
  const int a = tid / TILE, b = tid - a * TILE;
  if (t.a0 + a >= g.L[t.mu] || t.b0 + b >= g.L[t.nu]) return false;
  *lex = t.outside + (size_t)(t.a0 + a) * t.smu + (size_t)(t.b0 + b) * t.snu;
  const int x = (a + 1) * EXT + (b + 1);          // this site in the staged neighbourhood
  constexpr int PM = EXT, PN = 1;                 // one step in mu / nu there
  // the four leaves in the reference's order of factors (src/dirac.c:304-358); only the anti-Hermitian part of their sum is kept
#pragma unroll
  for (int r = 0; r < 9; r++) F[r] = 0.0;
  auto add = [&](const M3& l) {
#pragma unroll
    for (int i = 0; i < 3; i++) F[i] += l.a[4 * i].i + l.a[4 * i].i;
    int k = 3;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = i + 1; j < 3; j++, k += 2) { F[k] += l.a[3 * i + j].r - l.a[3 * j + i].r; F[k + 1] += l.a[3 * i + j].i + l.a[3 * j + i].i; }
  };
  M3 l = mul(mul(mul(staged(lds, 0, x), staged(lds, 1, x + PM)), dag(staged(lds, 0, x + PN))), dag(staged(lds, 1, x)));
  *plaq = l.a[0].r + l.a[4].r + l.a[8].r;
  add(l);
  add(mul(mul(mul(staged(lds, 1, x), dag(staged(lds, 0, x + PN - PM))), dag(staged(lds, 1, x - PM))), staged(lds, 0, x - PM)));
  add(mul(mul(mul(dag(staged(lds, 0, x - PM)), dag(staged(lds, 1, x - PM - PN))), staged(lds, 0, x - PM - PN)), staged(lds, 1, x - PN)));
  add(mul(mul(mul(dag(staged(lds, 1, x - PN)), staged(lds, 0, x - PN)), staged(lds, 1, x - PN + PM)), dag(staged(lds, 0, x))));
  // F = (Q - Q^dagger) / 16
#pragma unroll
  for (int r = 0; r < 9; r++) F[r] /= 16.0;
  return true;
}

struct GammaProducts { double re[6][16], im[6][16]; };   // gamma_mu gamma_nu for the six planes mu < nu

// the clover term of one site, 42 complex in the reference's packing (src/dirac.c:386-398), from the six F of the site:
// Fs[(p * 9 + r) * V + lex]
DDAMG_FS_HD void site_clover(const double* __restrict__ Fs, size_t V, size_t lex, double m0, double csw, const GammaProducts& gp,
                             double* __restrict__ out) {
  double clr[42], cli[42];
#pragma unroll
  for (int k = 0; k < 42; k++) { clr[k] = k < 12 ? 4.0 + m0 : 0.0; cli[k] = 0.0; }
#pragma unroll
  for (int p = 0; p < 6; p++) {
    double f[9];
#pragma unroll
    for (int r = 0; r < 9; r++) f[r] = Fs[((size_t)p * 9 + r) * V + lex];
    cplx qd[9];
    qd[0] = cplx{0.0, f[0]}; qd[4] = cplx{0.0, f[1]}; qd[8] = cplx{0.0, f[2]};
    qd[1] = cplx{f[3], f[4]}; qd[3] = cplx{-f[3], f[4]};
    qd[2] = cplx{f[5], f[6]}; qd[6] = cplx{-f[5], f[6]};
    qd[5] = cplx{f[7], f[8]}; qd[7] = cplx{-f[7], f[8]};
    // tensor = -csw * (gamma_mu gamma_nu) (x) F; the diagonal and the strict upper parts of both 6x6 blocks
    auto add = [&](int k, int i, int j) {
      const int gi = 4 * (i / 3) + (j / 3), c = 3 * (i % 3) + (j % 3);
      const double gr = gp.re[p][gi], gm = gp.im[p][gi];
      clr[k] += -csw * (gr * qd[c].r - gm * qd[c].i);
      cli[k] += -csw * (gr * qd[c].i + gm * qd[c].r);
    };
#pragma unroll
    for (int k = 0; k < 12; k++) add(k, k, k);
    int k = 12;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = i + 1; j < 6; j++, k++) add(k, i, j);
#pragma unroll
    for (int i = 6; i < 12; i++)
#pragma unroll
      for (int j = i + 1; j < 12; j++, k++) add(k, i, j);
  }
#pragma unroll
  for (int k = 0; k < 42; k++) { out[lex * 84 + 2 * k] = clr[k]; out[lex * 84 + 2 * k + 1] = cli[k]; }
}

}  // namespace fs
}  // namespace ddamg
