// lime.cpp -- ILDG configurations and SciDAC/ETMC spinors in the LIME container, see include/ddamg_hip_io.h.  Host code only; the
// container is read and written here directly (the reference links the c-lime library for it, src/lime_io.c).
#include "../../include/ddamg_hip_io.h"
#include "io_common.h"
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <cstdarg>
#include <string>
#include <vector>
#include <fcntl.h>
#include <unistd.h>

using namespace ddamg_io;

namespace {

const size_t LIME_HEADER = 144;
const unsigned char LIME_MAGIC[4] = {0x45, 0x67, 0x89, 0xab};
const size_t MAX_TEXT = 1u << 20;   // format and info records are a few hundred bytes

size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }

uint64_t load_be64(const unsigned char* b) { uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | b[i]; return v; }
void store_be64(unsigned char* b, uint64_t v) { for (int i = 7; i >= 0; i--) { b[i] = (unsigned char)(v & 0xff); v >>= 8; } }

uint64_t swapped(uint64_t v) { return __builtin_bswap64(v); }
uint32_t swapped(uint32_t v) { return __builtin_bswap32(v); }

// n big-endian numbers of the file -> doubles (fp32 widened exactly), and back (fp32: rounded to nearest)
template <typename Bits, typename Real>
void decode(const unsigned char* src, double* dst, size_t n) {
  for (size_t i = 0; i < n; i++) {
    Bits b; memcpy(&b, src + i * sizeof(Bits), sizeof b); b = swapped(b);
    Real r; memcpy(&r, &b, sizeof r);
    if (sizeof(Real) == sizeof(double)) memcpy(dst + i, &b, sizeof(double));   // bit patterns pass through
    else dst[i] = (double)r;
  }
}
template <typename Bits, typename Real>
void encode(const double* src, unsigned char* dst, size_t n) {
  for (size_t i = 0; i < n; i++) {
    Bits b;
    if (sizeof(Real) == sizeof(double)) memcpy(&b, src + i, sizeof b);
    else { const Real r = (Real)src[i]; memcpy(&b, &r, sizeof b); }
    b = swapped(b);
    memcpy(dst + i * sizeof(Bits), &b, sizeof b);
  }
}
void decode_reals(int precision, const unsigned char* src, double* dst, size_t n) {
  if (precision == 64) decode<uint64_t, double>(src, dst, n); else decode<uint32_t, float>(src, dst, n);
}
void encode_reals(int precision, const double* src, unsigned char* dst, size_t n) {
  if (precision == 64) encode<uint64_t, double>(src, dst, n); else encode<uint32_t, float>(src, dst, n);
}

// the integer behind `tag` in a record's text (lime_getParam + sscanf("%i"), src/lime_io.c:78-92,115-119)
bool tagged_int(const std::string& text, const char* tag, int* out) {
  const size_t pos = text.find(tag);
  if (pos == std::string::npos) return false;
  const char* s = text.c_str() + pos + strlen(tag);
  char* end = nullptr;
  const long v = strtol(s, &end, 0);
  if (end == s) return false;
  *out = (int)v;
  return true;
}

struct Format {            // an "ildg-format" or "etmc-*-format" record
  bool present = false, complete = false;
  int precision = 0, l[4] = {0, 0, 0, 0};   // T,Z,Y,X
  int flavours = 1, spin = 4, colour = 3;   // what the reference assumes when a tag is missing (src/lime_io.c:100-101)
};

struct Scan {
  std::vector<std::string> types;
  std::vector<long long> offsets, lengths;   // data of every record
  Format ildg, etmc;
  bool has_plaq = false; double plaq = 0;
  long long conf_off = -1, conf_len = 0, vec_off = -1, vec_len = 0;
};

Format parse_format(const std::string& text, bool etmc) {
  Format f; f.present = true;
  bool ok = tagged_int(text, "<precision>", &f.precision);
  ok = tagged_int(text, "<lx>", &f.l[3]) && ok;
  ok = tagged_int(text, "<ly>", &f.l[2]) && ok;
  ok = tagged_int(text, "<lz>", &f.l[1]) && ok;
  ok = tagged_int(text, "<lt>", &f.l[0]) && ok;
  if (etmc) { tagged_int(text, "<flavours>", &f.flavours); tagged_int(text, "<spin>", &f.spin); tagged_int(text, "<colour>", &f.colour); }
  f.complete = ok;
  return f;
}

int scan_file(const char* path, Scan& s) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail("cannot open LIME file '%s'", path);
  const off_t fsize = lseek(fd, 0, SEEK_END);
  int rc = 0;
  off_t off = 0;
  if (fsize < (off_t)sizeof LIME_MAGIC) rc = fail("'%s' is not a LIME file (shorter than the magic number)", path);
  while (rc == 0 && off < fsize) {
    unsigned char h[LIME_HEADER];
    const size_t have = (size_t)(fsize - off) < LIME_HEADER ? (size_t)(fsize - off) : LIME_HEADER;
    if (pread_all(fd, h, have, off)) { rc = fail("cannot read '%s'", path); break; }
    if (have >= sizeof LIME_MAGIC && memcmp(h, LIME_MAGIC, sizeof LIME_MAGIC) != 0) {
      rc = fail("'%s' is not a LIME file (no record header at byte %lld)", path, (long long)off); break;
    }
    if (have < LIME_HEADER) { rc = fail("LIME file '%s' ends early (inside the record header at byte %lld)", path, (long long)off); break; }
    const uint64_t len = load_be64(h + 8);
    h[LIME_HEADER - 1] = 0;
    const std::string type((const char*)h + 16);
    const off_t data = off + (off_t)LIME_HEADER;
    if (len > (uint64_t)(fsize - data)) {
      rc = fail("LIME file '%s' ends early (record '%s' states %llu bytes, %lld are left)", path, type.c_str(), (unsigned long long)len, (long long)(fsize - data));
      break;
    }
    s.types.push_back(type); s.offsets.push_back((long long)data); s.lengths.push_back((long long)len);
    const bool format = type == "ildg-format", etmc = type == "etmc-propagator-format" || type == "etmc-source-format", xlf = type == "xlf-info";
    if ((format || etmc || xlf) && len <= MAX_TEXT) {
      std::string text(len, '\0');
      if (len && pread_all(fd, &text[0], len, data)) { rc = fail("cannot read '%s'", path); break; }
      if (format) s.ildg = parse_format(text, false);
      if (etmc) s.etmc = parse_format(text, true);
      if (xlf) {
        const size_t pos = text.find("plaquette =");
        if (pos != std::string::npos) {
          const char* p = text.c_str() + pos + strlen("plaquette =");
          char* end = nullptr;
          const double v = strtod(p, &end);
          if (end != p) { s.has_plaq = true; s.plaq = v; }
        }
      }
    }
    if (type == "ildg-binary-data" && s.conf_off < 0) { s.conf_off = data; s.conf_len = (long long)len; }
    if (type == "scidac-binary-data" && s.vec_off < 0) { s.vec_off = data; s.vec_len = (long long)len; }
    off = data + (off_t)pad8(len);
  }
  close(fd);
  return rc;
}

void fill_info(const Scan& s, struct ddamg_hip_lime_info* out) {
  memset(out, 0, sizeof *out);
  const Format* f = nullptr;
  if (s.conf_off >= 0) { out->kind = 1; out->data_offset = s.conf_off; out->data_length = s.conf_len; f = &s.ildg; }
  else if (s.vec_off >= 0) { out->kind = 2; out->data_offset = s.vec_off; out->data_length = s.vec_len; f = &s.etmc; }
  if (f && f->present) { out->precision = f->precision; for (int mu = 0; mu < 4; mu++) out->lattice[mu] = f->l[mu]; }
  out->has_plaquette = s.has_plaq; out->plaquette = s.plaq;
  out->num_records = (int)s.types.size();
}

// lime_check_info (src/lime_io.c:152-161) on the format record `f` and the binary record of `len` bytes
int check_record(const char* path, const char* what, const Format& f, const int G[4], long long len, int reals_per_site) {
  if (!f.present) return fail("'%s' has no format record for its %s", path, what);
  if (!f.complete) return fail("'%s': incomplete format record (precision, lx, ly, lz and lt are needed)", path);
  if (f.precision != 32 && f.precision != 64) return fail("'%s': precision %d, only 32 and 64 are defined", path, f.precision);
  for (int mu = 0; mu < 4; mu++)
    if (f.l[mu] != G[mu]) return fail("%s '%s' is %dx%dx%dx%d, expected %dx%dx%dx%d (T,Z,Y,X)", what, path, f.l[0], f.l[1], f.l[2], f.l[3], G[0], G[1], G[2], G[3]);
  long long want = (long long)reals_per_site * (f.precision / 8);
  for (int mu = 0; mu < 4; mu++) want *= G[mu];
  if (len != want) return fail("'%s': the binary record has %lld bytes, a %dx%dx%dx%d %s in %d-bit precision has %lld", path, len, G[0], G[1], G[2], G[3], what, f.precision, want);
  return 0;
}

void record_header(unsigned char* h, const char* type, uint64_t len) {
  memset(h, 0, LIME_HEADER);
  memcpy(h, LIME_MAGIC, sizeof LIME_MAGIC);
  h[4] = 0; h[5] = 1;   // version
  h[6] = 0xC0;          // message begin + message end
  store_be64(h + 8, len);
  strncpy((char*)h + 16, type, 127);
}

// the records before the binary one, their padding and the binary record's header: every process computes the same bytes,
// so all of them know where the data starts without talking to each other
std::string preamble(const std::vector<std::pair<const char*, std::string>>& texts, const char* binary_type, uint64_t binary_len) {
  std::string out;
  unsigned char h[LIME_HEADER];
  for (const auto& t : texts) {
    record_header(h, t.first, t.second.size());
    out.append((const char*)h, LIME_HEADER);
    out += t.second;
    out.append(pad8(t.second.size()) - t.second.size(), '\0');
  }
  record_header(h, binary_type, binary_len);
  out.append((const char*)h, LIME_HEADER);
  return out;
}

std::string text_of(const char* fmt, ...) {
  char buf[2048];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  return buf;
}

// origin: the preamble and, where the record's length is no multiple of 8, the zeros behind it
int write_frame(int fd, const char* path, const std::string& pre, uint64_t binary_len) {
  if (pwrite_all(fd, pre.data(), pre.size(), 0)) return fail("write to '%s' failed", path);
  const char zeros[8] = {0};
  const size_t pad = pad8(binary_len) - binary_len;
  if (pad && pwrite_all(fd, zeros, pad, (off_t)(pre.size() + binary_len))) return fail("write to '%s' failed", path);
  return 0;
}

}  // namespace

int ddamg_io::ildg_checked_info(const char* path, const int G[4], struct ddamg_hip_lime_info* info) {
  Scan s;
  if (scan_file(path, s)) return -1;
  if (s.conf_off < 0) return fail("'%s' has no binary record 'ildg-binary-data'", path);
  if (check_record(path, "configuration", s.ildg, G, s.conf_len, 72)) return -1;
  fill_info(s, info);
  return 0;
}

extern "C" {

int ddamg_hip_lime_info(const char* path, struct ddamg_hip_lime_info* out) {
  Scan s;
  if (!path || !out) return fail("lime_info: null argument");
  if (scan_file(path, s)) return -1;
  fill_info(s, out);
  return 0;
}

int ddamg_hip_read_ildg_conf(const char* path, const int G[4], const int P[4], const int C[4], double* gauge_local, double* plaq_out, int* has_plaq_out) {
  Part p;
  if (!make_part(G, P, C, p)) return fail("read_ildg_conf: process grid does not divide the lattice / coordinates outside the grid");
  struct ddamg_hip_lime_info info;
  if (ildg_checked_info(path, G, &info)) return -1;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail("cannot open LIME file '%s'", path);
  const size_t bytes = info.precision / 8, row_reals = (size_t)72 * p.L[3];
  std::vector<unsigned char> raw(row_reals * bytes);
  std::vector<double> row(row_reals);
  const int rc = for_rows(p, [&](size_t r, size_t gsite) {
    if (pread_all(fd, raw.data(), raw.size(), (off_t)(info.data_offset + (long long)(gsite * 72 * bytes)))) return fail("LIME file '%s' ends early", path);
    decode_reals(info.precision, raw.data(), row.data(), row_reals);
    double* dst = gauge_local + r * row_reals;
    for (int x = 0; x < p.L[3]; x++)          // X,Y,Z,T -> T,Z,Y,X: the four 18-real groups of a site reversed
      for (int mu = 0; mu < 4; mu++) memcpy(dst + (size_t)x * 72 + (3 - mu) * 18, row.data() + (size_t)x * 72 + mu * 18, 18 * sizeof(double));
    return 0;
  });
  close(fd);
  if (rc == 0 && plaq_out) *plaq_out = 3.0 * info.plaquette;
  if (rc == 0 && has_plaq_out) *has_plaq_out = info.has_plaquette;
  return rc;
}

int ddamg_hip_write_ildg_conf(const char* path, const int G[4], const int P[4], const int C[4], int precision, const double* gauge_local, double plaq) {
  Part p;
  if (!make_part(G, P, C, p)) return fail("write_ildg_conf: process grid does not divide the lattice / coordinates outside the grid");
  if (precision != 32 && precision != 64) return fail("write_ildg_conf: precision must be 32 or 64");
  const size_t bytes = precision / 8;
  const uint64_t len = (uint64_t)p.Vglob * 72 * bytes;
  const std::string format = text_of("<?xml version=\"1.0\" encoding=\"UTF-8\"?>\n<ildgFormat xmlns=\"http://www.lqcd.org/ildg\" "
                                     "xmlns:xsi=\"http://www.w3.org/2001/XMLSchema-instance\" xsi:schemaLocation=\"http://www.lqcd.org/ildg filefmt.xsd\">\n"
                                     "  <version>1.0</version>\n  <field>su3gauge</field>\n  <precision>%d</precision>\n"
                                     "  <lx>%d</lx>\n  <ly>%d</ly>\n  <lz>%d</lz>\n  <lt>%d</lt>\n</ildgFormat>", precision, G[3], G[2], G[1], G[0]);
  const std::string pre = preamble({{"ildg-format", format}, {"xlf-info", text_of("plaquette = %.17g\n", plaq / 3.0)}}, "ildg-binary-data", len);
  const int fd = open(path, O_WRONLY | O_CREAT, 0644);
  if (fd < 0) return fail("cannot create '%s'", path);
  int rc = at_origin(p) ? write_frame(fd, path, pre, len) : 0;
  const size_t row_reals = (size_t)72 * p.L[3];
  std::vector<unsigned char> raw(row_reals * bytes);
  std::vector<double> row(row_reals);
  if (rc == 0) rc = for_rows(p, [&](size_t r, size_t gsite) {
    const double* src = gauge_local + r * row_reals;
    for (int x = 0; x < p.L[3]; x++)
      for (int mu = 0; mu < 4; mu++) memcpy(row.data() + (size_t)x * 72 + (3 - mu) * 18, src + (size_t)x * 72 + mu * 18, 18 * sizeof(double));
    encode_reals(precision, row.data(), raw.data(), row_reals);
    if (pwrite_all(fd, raw.data(), raw.size(), (off_t)(pre.size() + gsite * 72 * bytes))) return fail("write to '%s' failed", path);
    return 0;
  });
  close(fd);
  return rc;
}

int ddamg_hip_read_lime_vector(const char* path, const int G[4], const int P[4], const int C[4], double* vector_local) {
  Part p;
  if (!make_part(G, P, C, p)) return fail("read_lime_vector: process grid does not divide the lattice / coordinates outside the grid");
  Scan s;
  if (scan_file(path, s)) return -1;
  if (s.vec_off < 0) return fail("'%s' has no binary record 'scidac-binary-data'", path);
  if (s.etmc.present && (s.etmc.flavours != 1 || s.etmc.spin != 4 || s.etmc.colour != 3))
    return fail("'%s' holds flavours %d, spin %d, colour %d: only flavours 1, spin 4, colour 3 is read", path, s.etmc.flavours, s.etmc.spin, s.etmc.colour);
  if (check_record(path, "vector", s.etmc, G, s.vec_len, 24)) return -1;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail("cannot open LIME file '%s'", path);
  const size_t bytes = s.etmc.precision / 8, row_reals = (size_t)24 * p.L[3];
  std::vector<unsigned char> raw(row_reals * bytes);
  const int rc = for_rows(p, [&](size_t r, size_t gsite) {
    if (pread_all(fd, raw.data(), raw.size(), (off_t)(s.vec_off + (long long)(gsite * 24 * bytes)))) return fail("LIME file '%s' ends early", path);
    decode_reals(s.etmc.precision, raw.data(), vector_local + r * row_reals, row_reals);
    return 0;
  });
  close(fd);
  return rc;
}

int ddamg_hip_write_lime_vector(const char* path, const int G[4], const int P[4], const int C[4], const ddamg_hip_vector_header* header, const double* vector_local) {
  Part p;
  if (!make_part(G, P, C, p)) return fail("write_lime_vector: process grid does not divide the lattice / coordinates outside the grid");
  const ddamg_hip_vector_header none = {nullptr, 0, 0, 0, 0, nullptr, nullptr, 0, nullptr};
  const ddamg_hip_vector_header& h = header ? *header : none;
  const uint64_t len = (uint64_t)p.Vglob * 24 * sizeof(double);
  // lime_write_info, src/lime_io.c:163-217; of its "dd_alpha_amg-header" the lines that ddamg_hip_vector_header has fields for
  const std::string format = text_of("<?xml version=\"1.0\" encoding=\"UTF-8\"?>\n<etmcFormat>\n\t<field>diracFermion</field>\n\t<precision>64</precision>\n"
                                     "\t<flavours>1</flavours>\n\t<lx>%d</lx>\n\t<ly>%d</ly>\n\t<lz>%d</lz>\n\t<lt>%d</lt>\n\t<spin>4</spin>\n\t<colour>3</colour>\n"
                                     "</etmcFormat>", G[3], G[2], G[1], G[0]);
  const std::string text = text_of("<header>\n\tclifford basis: %s\n\tm0: %.14lf\n\tcsw: %.14lf\n\tclov plaq: %.14lf\n\thopp plaq: %.14lf\n"
                                   "\tclov conf name: %s\n\thopp conf name: %s\n\tX: %d\n\tY: %d\n\tZ: %d\n\tT: %d\n"
                                   "\tX local: %d\n\tY local: %d\n\tZ local: %d\n\tT local: %d\n</header>",
                                   "BASIS0:OPENQCD/DD-HMC BASIS", h.m0, h.csw, h.clov_plaq, h.hopp_plaq, h.clov_conf_name ? h.clov_conf_name : "",
                                   h.hopp_conf_name ? h.hopp_conf_name : "", G[3], G[2], G[1], G[0], p.L[3], p.L[2], p.L[1], p.L[0]);
  const std::string pre = preamble({{"vector-type", "Vector_by_DDalphaAMG"}, {"etmc-propagator-format", format}, {"dd_alpha_amg-header", text}},
                                   "scidac-binary-data", len);
  const int fd = open(path, O_WRONLY | O_CREAT, 0644);
  if (fd < 0) return fail("cannot create '%s'", path);
  int rc = at_origin(p) ? write_frame(fd, path, pre, len) : 0;
  const size_t row_reals = (size_t)24 * p.L[3];
  std::vector<unsigned char> raw(row_reals * sizeof(double));
  if (rc == 0) rc = for_rows(p, [&](size_t r, size_t gsite) {
    encode_reals(64, vector_local + r * row_reals, raw.data(), row_reals);
    if (pwrite_all(fd, raw.data(), raw.size(), (off_t)(pre.size() + gsite * 24 * sizeof(double)))) return fail("write to '%s' failed", path);
    return 0;
  });
  close(fd);
  return rc;
}

}  // extern "C"
