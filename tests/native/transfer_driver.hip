// transfer_driver.hip -- host program that runs operations of Interpolation<T> (transfer.h) or CoarseTransfer<T> (coarse_mg.h) on
// arrays a test wrote, without a FineOp, a gauge field or a context.
//
//   transfer_driver <dir>
//
// <dir>/case.txt: cls (fine | coarse), type (float | double), L0..L3 B0..B3 A0..A3 (the level), Bc0..Bc3 (Schwarz blocks of the
// next level, whose lattice is L / A), nvec, n (coarse: dof of the level), the switches gs_workgroup / coarse_gs_global /
// coarse_gs_workgroup_form, sentinel, ops (comma separated, run in this order on one object) and what the operations name below.
// One process serves one (geometry, nvec, type); the batched operations loop over the calls listed in sel_<op>.bin.
//
// Fields cross the program boundary in LEXICOGRAPHIC site order: a fine vector is [V][24], a vector of a coarse level [V][n][2],
// of the type of the case.  The driver places them in the device layout (Geometry::site_of_lex; chunked SoA on the fine level) and
// writes lex_of_site of both geometries and agg_csite, so that the test can check the site order from coordinates alone.  Every
// buffer an operation writes is filled with `sentinel` first, 64 elements longer than the operation needs and with the strides
// of the case; out_<name>_gaps.bin holds every element of it that lies outside the vectors, in buffer order.
//
// The driver checks no result.  It refuses a case whose counts or strides would address outside the arrays it was given; a
// std::runtime_error of the library ends it with status 2 and the text on stderr.
#include "transfer.h"
#include "coarse_mg.h"
#include "driver_case.h"

using namespace ddamg;

// where real r of lexicographic site x of a field lies in a device vector; pos[x] < 0: the field does not hold that site
struct Layout {
  size_t V = 0;             // sites of the device field
  int nreal = 0, CH = 0;    // reals per site; chunk width of the chunked-SoA layout, 0: site-major (AoS)
  std::vector<long long> pos;
  size_t span() const { return V * (size_t)nreal; }
  size_t at(size_t s, int r) const { return CH ? ((size_t)(r / CH) * V + s) * CH + r % CH : s * nreal + r; }
};
static Layout layout_of(const Geometry& g, int nreal, int CH) {
  Layout l;
  l.V = (size_t)g.V; l.nreal = nreal; l.CH = CH;
  l.pos.assign(g.site_of_lex.begin(), g.site_of_lex.end());
  return l;
}

// `count` device vectors `stride` apart, filled with the sentinel, with a record of what belongs to a vector
template <typename T>
struct Buf {
  std::vector<T> h;
  std::vector<char> defined;
  DeviceBuffer<T> d;
  size_t stride = 0, count = 0;
  void init(size_t count_, size_t stride_, size_t span, T sentinel) {
    count = count_; stride = stride_;
    need(count <= 1 || stride >= span, "stride shorter than a vector");
    need(stride % 4 == 0, "strides must keep vectors 16-byte aligned");
    h.assign((count ? (count - 1) * stride + span : 0) + 64, sentinel);
    defined.assign(h.size(), 0);
  }
  void put(size_t v, const Layout& l, const T* lex) {     // lex: [sites in lexicographic order][nreal], or null: mark only
    need(v < count && v * stride + l.span() + 64 <= h.size(), "vector outside its buffer");
    for (size_t x = 0; x < l.pos.size(); x++) {
      if (l.pos[x] < 0) continue;
      for (int r = 0; r < l.nreal; r++) {
        const size_t o = v * stride + l.at((size_t)l.pos[x], r);
        if (lex) h[o] = lex[x * l.nreal + r];
        defined[o] = 1;
      }
    }
  }
  void up() { d.alloc(h.size()); DDAMG_HIP_CHECK(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice)); }
  void down() { DDAMG_HIP_CHECK(hipMemcpy(h.data(), d, sizeof(T) * h.size(), hipMemcpyDeviceToHost)); }
  // the vectors back in lexicographic order, and everything else in buffer order
  void store(const Case& c, const std::string& name, const Layout& l) {
    down();
    std::vector<T> lex(count * l.pos.size() * l.nreal), gaps;
    for (size_t v = 0; v < count; v++)
      for (size_t x = 0; x < l.pos.size(); x++)
        for (int r = 0; r < l.nreal; r++) lex[(v * l.pos.size() + x) * l.nreal + r] = l.pos[x] < 0 ? (T)0 : h[v * stride + l.at((size_t)l.pos[x], r)];
    for (size_t o = 0; o < h.size(); o++) if (!defined[o]) gaps.push_back(h[o]);
    c.write(name, lex.data(), lex.size());
    c.write(name + "_gaps", gaps.data(), gaps.size());
  }
};

static void sync(hipStream_t st) { DDAMG_HIP_CHECK(hipStreamSynchronize(st)); }

static std::vector<std::string> split(const std::string& s) {
  std::vector<std::string> v;
  std::stringstream ss(s);
  std::string tok;
  while (std::getline(ss, tok, ',')) if (!tok.empty()) v.push_back(tok);
  return v;
}

// the calls of a batched operation: sel_<op>.bin is int32 [calls][1 + selw_<op>], a count followed by pool indices
struct Calls {
  std::vector<int> sel;
  size_t w = 0, n = 0;
  Calls(const Case& c, const std::string& op, size_t npool) {
    sel = c.read<int>("sel_" + op);
    w = (size_t)c.i("selw_" + op);
    need(sel.size() % (1 + w) == 0, "sel_" + op + " is not [calls][1 + width]");
    n = sel.size() / (1 + w);
    for (size_t k = 0; k < n; k++) {
      need(count(k) >= 0 && (size_t)count(k) <= w, "sel_" + op + ": count outside the row");
      for (int q = 0; q < count(k); q++) need(col(k, q) >= 0 && (size_t)col(k, q) < npool, "sel_" + op + ": column outside the pool");
    }
  }
  int count(size_t k) const { return sel[k * (1 + w)]; }
  int col(size_t k, int q) const { return sel[k * (1 + w) + 1 + q]; }
};

template <typename T>
static void run_fine(const Case& c, const Geometry& g, const Geometry& gc, const Knobs& knobs, hipStream_t st) {
  constexpr int CH = Chunk<T>::CH;
  const int nvec = (int)c.i("nvec");
  need(nvec >= 1 && nvec <= 64, "1 <= nvec <= 64");
  const T sentinel = (T)c.d("sentinel", 7.5);
  Interpolation<T> ip;
  ip.alloc(g, gc, nvec, knobs);
  {
    std::vector<int> ac((size_t)ip.num_aggs);
    DDAMG_HIP_CHECK(hipMemcpy(ac.data(), ip.agg_csite, sizeof(int) * ac.size(), hipMemcpyDeviceToHost));
    c.write("agg_csite", ac.data(), ac.size());
  }
  const Layout F = layout_of(g, 24, CH), C = layout_of(gc, 4 * nvec, 0);
  const size_t fsz = F.span(), csz = C.span(), nlex = (size_t)g.V * 24, nclex = (size_t)gc.V * 4 * nvec;
  if (c.i("have_P", 0)) {
    const std::vector<T> P = c.read<T>("P");
    need(P.size() == nvec * nlex, "P is not [nvec][V][24]");
    for (int j = 0; j < nvec; j++) {
      Buf<T> col;
      col.init(1, fsz, fsz, sentinel);
      col.put(0, F, P.data() + (size_t)j * nlex);
      col.up();
      ip.set_column(j, col.d, st);
      sync(st);
    }
  }
  std::vector<T> pool;      // fine fields of the batched restrictions, read once
  std::string pool_name;
  const auto fine_pool = [&](const std::string& name, size_t per) {
    if (pool_name != name) { pool = c.read<T>(name); pool_name = name; }
    need(!pool.empty() && pool.size() % (per * nlex) == 0, name + " is not [pool]" + (per > 1 ? "[5]" : "") + "[V][24]");
    return pool.size() / (per * nlex);
  };
  for (const std::string& op : split(c.str("ops"))) {
    if (op == "none") {          // the geometry and agg_csite only
    } else if (op == "columns") {
      std::vector<T> raw(ip.p_elems());
      DDAMG_HIP_CHECK(hipMemcpy(raw.data(), ip.P, sizeof(T) * raw.size(), hipMemcpyDeviceToHost));
      c.write("Praw", raw.data(), raw.size());
      const size_t stride = (size_t)c.i("col_stride", (long long)fsz);
      Buf<T> out;
      out.init(nvec, stride, fsz, sentinel);
      for (int j = 0; j < nvec; j++) out.put(j, F, nullptr);
      out.up();
      for (int j = 0; j < nvec; j++) ip.get_column(j, out.d + (size_t)j * stride, st);
      sync(st);
      out.store(c, "cols", F);
    } else if (op == "restrict") {
      const std::vector<T> phi = c.read<T>("phi");
      need(phi.size() == nlex, "phi is not [V][24]");
      Buf<T> in, out;
      in.init(1, fsz, fsz, sentinel); in.put(0, F, phi.data()); in.up();
      out.init(1, csz, csz, sentinel); out.put(0, C, nullptr); out.up();
      ip.restrict_to(out.d, in.d, st);
      sync(st);
      out.store(c, "restrict", C);
    } else if (op == "restrict5") {
      const std::vector<T> phi = c.read<T>("phi5");
      need(phi.size() == 5 * nlex, "phi5 is not [5][V][24]");
      const size_t is = (size_t)c.i("in_stride", (long long)fsz), os = (size_t)c.i("out_stride", (long long)csz);
      Buf<T> in, out;
      in.init(5, is, fsz, sentinel); out.init(5, os, csz, sentinel);
      for (int m = 0; m < 5; m++) { in.put(m, F, phi.data() + (size_t)m * nlex); out.put(m, C, nullptr); }
      in.up(); out.up();
      ip.restrict5(out.d, os, in.d, is, st);
      sync(st);
      out.store(c, "restrict5", C);
    } else if (op == "interp" || op == "interp_add") {
      const bool add = op == "interp_add";
      const std::vector<T> pc = c.read<T>("phic");
      need(pc.size() == nclex, "phic is not [Vc][2 nvec][2]");
      std::vector<T> phi0;
      if (add) { phi0 = c.read<T>("phi0"); need(phi0.size() == nlex, "phi0 is not [V][24]"); }
      Buf<T> in, out;
      in.init(1, csz, csz, sentinel); in.put(0, C, pc.data()); in.up();
      out.init(1, fsz, fsz, sentinel); out.put(0, F, add ? phi0.data() : nullptr); out.up();
      ip.interpolate(out.d, in.d, add, st);
      sync(st);
      out.store(c, op, F);
    } else if (op == "rbatch" || op == "rslab") {
      const bool slab = op == "rslab";
      const size_t npool = fine_pool("W", 1);
      const Calls calls(c, op, npool);
      const int agg0 = slab ? (int)c.i("agg0") : 0, naggs = slab ? (int)c.i("naggs") : g.num_aggs;
      Layout S = F;         // the slab's fields hold the sites of the aggregates [agg0, agg0 + naggs) only
      if (slab) {
        need(agg0 >= 0 && naggs >= 1 && agg0 + naggs <= g.num_aggs, "slab outside the aggregates");
        S.V = (size_t)naggs * g.agg_sites;
        for (auto& p : S.pos) { p -= (long long)agg0 * g.agg_sites; if (p >= (long long)S.V) p = -1; }
      }
      const size_t is = (size_t)c.i("in_stride_" + op, (long long)S.span()), os = (size_t)c.i("out_stride_" + op, (long long)csz);
      for (size_t k = 0; k < calls.n; k++) {
        const int nw = calls.count(k);
        Buf<T> in, out;
        in.init(nw, is, S.span(), sentinel); out.init(nw, os, csz, sentinel);
        for (int q = 0; q < nw; q++) { in.put(q, S, pool.data() + (size_t)calls.col(k, q) * nlex); out.put(q, C, nullptr); }
        in.up(); out.up();
        if (slab) ip.restrict_batch_slab(out.d, os, in.d, is, nw, agg0, naggs, st);
        else ip.restrict_batch(out.d, os, in.d, is, nw, st);
        sync(st);
        out.store(c, op + "_" + std::to_string(k), C);
      }
    } else if (op == "rcompact") {
      const size_t npool = fine_pool("W5", 5);
      const Calls calls(c, op, npool);
      const int agg0 = (int)c.i("agg0", 0), naggs = (int)c.i("naggs", g.num_aggs), S = g.agg_sites;
      need(agg0 >= 0 && naggs >= 1 && agg0 + naggs <= g.num_aggs, "slab outside the aggregates");
      AggFaces af;
      std::vector<unsigned short> tab;
      need(agg_face_tables(g, af, tab), "the aggregates have no common face tables");
      DeviceBuffer<unsigned short> d_tab;
      d_tab.upload(tab);
      af.rank = d_tab; af.list = d_tab + (size_t)4 * S;
      const unsigned short* list = tab.data() + (size_t)4 * S;
      const size_t wstride = (size_t)24 * af.column_sites((size_t)naggs);
      const bool direct = c.i("mdirect", 0) != 0;
      const int nt2 = (int)c.i("nt2", 0);
      const std::vector<long long> col_bases = c.has("col_bases") ? c.list("col_bases") : std::vector<long long>();   // one per call
      const size_t msize2 = (size_t)c.i("msize2", 0), os = (size_t)c.i("out_stride_rcompact", (long long)csz);
      for (size_t k = 0; k < calls.n; k++) {
        const int ncols = calls.count(k), col_base = k < col_bases.size() ? (int)col_bases[k] : 0;
        // column q: the self part on all sites of the slab's aggregates, then the forward part of every direction on its face
        // sites in the order of the face list, each part a chunked field of its own
        std::vector<T> w((size_t)ncols * wstride + 64, sentinel);
        for (int q = 0; q < ncols; q++)
          for (int p = 0; p < 5; p++) {
            const size_t ks = p == 0 ? (size_t)S : (size_t)af.nface[p - 1], Vw = (size_t)naggs * ks, woff = (size_t)24 * af.part_offset_sites(p, (size_t)naggs);
            const T* src = pool.data() + ((size_t)calls.col(k, q) * 5 + p) * nlex;
            for (int ai = 0; ai < naggs; ai++)
              for (size_t e = 0; e < ks; e++) {
                const int i = p == 0 ? (int)e : (int)list[af.loff[p - 1] + e];
                const size_t x = (size_t)g.lex_of_site[(size_t)(agg0 + ai) * S + i];
                for (int r = 0; r < 24; r++) {
                  const size_t o = (size_t)q * wstride + woff + ((size_t)(r / CH) * Vw + (size_t)ai * ks + e) * CH + r % CH;
                  need(o < w.size() - 64, "compact field outside its column");
                  w[o] = src[x * 24 + r];
                }
              }
          }
        Dev<T> W;
        W.from(w);
        Buf<T> out;
        out.init(direct ? 0 : (size_t)5 * ncols, os, csz, sentinel);
        for (size_t v = 0; v < out.count; v++) out.put(v, C, nullptr);
        out.up();
        Dev<T> M;
        if (direct) {
          need(nt2 >= 1 && (size_t)((2 * nvec + 7) / 8) * nt2 * 64 <= msize2 && col_base >= 0 && col_base + ncols <= 8 * nt2, "columns outside the matrices");
          M.from(std::vector<T>((size_t)gc.V * 5 * msize2 * 2, sentinel));
        }
        ip.restrict_batch_compact(out.d, os, W.p, ncols, af, agg0, naggs, st, direct ? (T*)M.p : nullptr, nt2, msize2, col_base);
        sync(st);
        if (direct) M.store(c, "mdirect_" + std::to_string(k));
        else out.store(c, "rcompact_" + std::to_string(k), C);
      }
    } else if (op == "ibatch") {
      const std::vector<T> cp = c.read<T>("C");
      need(!cp.empty() && cp.size() % nclex == 0, "C is not [pool][Vc][2 nvec][2]");
      const Calls calls(c, op, cp.size() / nclex);
      const size_t is = (size_t)c.i("c_stride", (long long)csz), os = (size_t)c.i("out_stride_ibatch", (long long)fsz);
      for (size_t k = 0; k < calls.n; k++) {
        const int nrhs = calls.count(k);
        Buf<T> in, out;
        in.init(nrhs, is, csz, sentinel); out.init(nrhs, os, fsz, sentinel);
        for (int q = 0; q < nrhs; q++) { in.put(q, C, cp.data() + (size_t)calls.col(k, q) * nclex); out.put(q, F, nullptr); }
        in.up(); out.up();
        ip.interpolate_batch(out.d, os, in.d, is, nrhs, st);
        sync(st);
        out.store(c, "ibatch_" + std::to_string(k), F);
      }
    } else if (op == "gs") {
      const std::vector<T> tv = c.read<T>("tv");
      need(tv.size() == nvec * nlex, "tv is not [nvec][V][24]");
      Buf<T> in, out;
      in.init(nvec, ip.pstride, fsz, sentinel); out.init(nvec, fsz, fsz, sentinel);
      for (int j = 0; j < nvec; j++) { in.put(j, F, tv.data() + (size_t)j * nlex); out.put(j, F, nullptr); }
      DDAMG_HIP_CHECK(hipMemcpy(ip.tv, in.h.data(), sizeof(T) * ip.pstride * nvec, hipMemcpyHostToDevice));
      ip.orthonormalize(st);
      sync(st);
      out.up();
      for (int j = 0; j < nvec; j++) ip.get_column(j, out.d + (size_t)j * fsz, st);
      sync(st);
      out.store(c, "gs", F);
    } else need(false, "unknown operation " + op);
  }
}

template <typename T>
static void run_coarse(const Case& c, const Geometry& g, const Geometry& gc, const Knobs& knobs, hipStream_t st) {
  const int nvec = (int)c.i("nvec"), n = (int)c.i("n");
  need(nvec >= 1 && nvec <= 64 && n >= 2 && n % 2 == 0 && n <= 128, "1 <= nvec <= 64, n even, 2 <= n <= 128");
  const T sentinel = (T)c.d("sentinel", 7.5);
  CoarseTransfer<T> ct;
  ct.alloc(g, gc, n, nvec, knobs);
  {
    std::vector<int> ac((size_t)ct.num_aggs);
    DDAMG_HIP_CHECK(hipMemcpy(ac.data(), ct.agg_csite, sizeof(int) * ac.size(), hipMemcpyDeviceToHost));
    c.write("agg_csite", ac.data(), ac.size());
  }
  const Layout A = layout_of(g, 2 * n, 0), C = layout_of(gc, 4 * nvec, 0);
  const size_t asz = A.span(), csz = C.span();
  need(ct.pstride == asz, "pstride is not one vector");
  const auto vectors_to = [&](T* dst, const std::string& name) {
    const std::vector<T> v = c.read<T>(name);
    need(v.size() == nvec * asz, name + " is not [nvec][V][n][2]");
    Buf<T> b;
    b.init(nvec, asz, asz, sentinel);
    for (int j = 0; j < nvec; j++) b.put(j, A, v.data() + (size_t)j * asz);
    DDAMG_HIP_CHECK(hipMemcpy(dst, b.h.data(), sizeof(T) * asz * nvec, hipMemcpyHostToDevice));
  };
  if (c.i("have_P", 0)) vectors_to(ct.P, "P");
  for (const std::string& op : split(c.str("ops"))) {
    if (op == "none") {
    } else if (op == "c_restrict") {
      const std::vector<T> phi = c.read<T>("phi");
      need(phi.size() == asz, "phi is not [V][n][2]");
      Buf<T> in, out;
      in.init(1, asz, asz, sentinel); in.put(0, A, phi.data()); in.up();
      out.init(1, csz, csz, sentinel); out.put(0, C, nullptr); out.up();
      ct.restrict_to(out.d, in.d, st);
      sync(st);
      out.store(c, op, C);
    } else if (op == "c_interp" || op == "c_interp_add") {
      const bool add = op == "c_interp_add";
      const std::vector<T> pc = c.read<T>("phic");
      need(pc.size() == csz, "phic is not [Vc][2 nvec][2]");
      std::vector<T> phi0;
      if (add) { phi0 = c.read<T>("phi0"); need(phi0.size() == asz, "phi0 is not [V][n][2]"); }
      Buf<T> in, out;
      in.init(1, csz, csz, sentinel); in.put(0, C, pc.data()); in.up();
      out.init(1, asz, asz, sentinel); out.put(0, A, add ? phi0.data() : nullptr); out.up();
      ct.interpolate(out.d, in.d, add, st);
      sync(st);
      out.store(c, op, A);
    } else if (op == "c_gs") {
      vectors_to(ct.tv, "tv");
      ct.orthonormalize((int)c.i("passes"), st);
      sync(st);
      Buf<T> out;
      out.init(nvec, asz, asz, sentinel);
      for (int j = 0; j < nvec; j++) out.put(j, A, nullptr);
      out.d.alloc(out.h.size());
      DDAMG_HIP_CHECK(hipMemcpy(out.d, out.h.data(), sizeof(T) * out.h.size(), hipMemcpyHostToDevice));
      DDAMG_HIP_CHECK(hipMemcpy(out.d, ct.P, sizeof(T) * asz * nvec, hipMemcpyDeviceToDevice));
      out.store(c, op, A);
    } else need(false, "unknown operation " + op);
  }
}

int main(int argc, char** argv) {
  driver_name = "transfer_driver";
  if (argc != 2) { fprintf(stderr, "usage: transfer_driver <case directory>\n"); return 64; }
  try {
    const Case c(argv[1]);
    int L[4], B[4], A[4], Lc[4], Bc[4];
    for (int mu = 0; mu < 4; mu++) {
      const std::string m = std::to_string(mu);
      L[mu] = (int)c.i("L" + m); B[mu] = (int)c.i("B" + m); A[mu] = (int)c.i("A" + m); Bc[mu] = (int)c.i("Bc" + m);
      need(L[mu] >= 1 && A[mu] >= 1 && L[mu] % A[mu] == 0, "the aggregates must tile the lattice");
      Lc[mu] = L[mu] / A[mu];
    }
    Geometry g, gc;
    g.build(L, B, A);
    gc.build(Lc, Bc, Lc);
    need(g.V <= 65536, "at most 65536 sites");
    c.write("lex_of_site", g.lex_of_site.data(), g.lex_of_site.size());
    c.write("lex_of_site_c", gc.lex_of_site.data(), gc.lex_of_site.size());
    Knobs knobs;              // from the case, never from the environment
    knobs.gs_workgroup = c.i("gs_workgroup", 0) != 0;
    knobs.coarse_gs_global = c.i("coarse_gs_global", 0) != 0;
    knobs.coarse_gs_workgroup_form = c.i("coarse_gs_workgroup_form", 0) != 0;
    hipStream_t st;
    DDAMG_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const std::string cls = c.str("cls"), type = c.str("type");
    need(type == "float" || type == "double", "type must be float or double");
    if (cls == "fine") { if (type == "float") run_fine<float>(c, g, gc, knobs, st); else run_fine<double>(c, g, gc, knobs, st); }
    else if (cls == "coarse") { if (type == "float") run_coarse<float>(c, g, gc, knobs, st); else run_coarse<double>(c, g, gc, knobs, st); }
    else need(false, "cls must be fine or coarse");
    DDAMG_HIP_CHECK(hipStreamSynchronize(st));
    DDAMG_HIP_CHECK(hipStreamDestroy(st));
  } catch (const std::runtime_error& e) {
    fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  return 0;
}
