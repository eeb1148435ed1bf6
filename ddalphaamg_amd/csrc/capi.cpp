// capi.cpp -- implementation of the thin C-ABI (include/ddamg_hip.h).
#include "capi_common.h"
#include "gauge.h"
#include "storage_refusal.h"
#include "ildg_device.h"
#include "io_common.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <fcntl.h>

using namespace ddamg;

thread_local std::string g_ddamg_last_error;

ddamg_hip_ctx::~ddamg_hip_ctx() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  mg32.reset(); mg64.reset();
  if (comm) comm_destroy(comm);
}

double* ddamg_hip_ctx::stage(size_t bytes) {
  if (bytes > d_stage.bytes()) d_stage.alloc(bytes / sizeof(double));   // every caller stages fp64 numbers
  return d_stage;
}

// why this context cannot keep what `kind` names in 16 bits (nullptr: it can): storage_refusal.h on the context's parameters
static const char* storage_refusal(const ddamg_hip_ctx* c, StorageKind kind) {
  const ddamg_hip_params& p = c->par;
  if (kind == Coarse) return coarse_half_refusal(p.num_levels, p.method, p.mixed_precision, p.odd_even, c->levels.back()->geom.distributed(), p.gather_coarsest != 0);
  if (kind == Transfer) return transfer_half_refusal(p.num_levels, p.method, p.mixed_precision);
  bool decomposed = false;
  for (int l = 1; l + 1 < p.num_levels; l++) decomposed = decomposed || c->levels[l]->geom.distributed();
  return intermediate_half_refusal(p.num_levels, p.method, p.mixed_precision, decomposed);
}

// ddamg_hip_set_coarse_storage / _transfer_ / _intermediate_: name is the word their messages begin with
static int set_storage(ddamg_hip_ctx* c, StorageKind kind, int bits, const char* name) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(bits == 16 || bits == 32, (std::string(name) + " storage: bits must be 16 or 32").c_str());
  if (bits == 16) if (const char* why = storage_refusal(c, kind)) throw std::runtime_error(why);
  if (c->mg32) c->mg32->set_storage(kind, bits);
  c->storage.bits[kind] = bits;
  DDAMG_API_END
}

void ddamg_require_device_array(const ddamg_hip_ctx* c, const void* p, size_t bytes, const char* what) {
  const std::string name(what);
  DDAMG_REQUIRE(p != nullptr, (name + ": null pointer where an array in device memory is expected").c_str());
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) (void)hipGetLastError();   // a pointer the runtime does not know: host memory
  DDAMG_REQUIRE(e == hipSuccess && at.type == hipMemoryTypeDevice,
                (name + ": not a pointer into device memory (host arrays go through the entry point without _device)").c_str());
  DDAMG_REQUIRE(at.device == c->device, (name + ": the array lies in the memory of another device than the context's").c_str());
  hipDeviceptr_t base = nullptr; size_t size = 0;
  const hipError_t r = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)const_cast<void*>(p));
  if (r != hipSuccess) (void)hipGetLastError();
  DDAMG_REQUIRE(r == hipSuccess && (const char*)p + bytes <= (const char*)base + size, (name + ": the device allocation is smaller than the array").c_str());
}

void ddamg_require_disjoint(const void* out, const void* in, size_t bytes, const char* what) {
  const char* a = (const char*)out; const char* b = (const char*)in;
  DDAMG_REQUIRE(a + bytes <= b || b + bytes <= a, (std::string(what) + ": the output and the input array overlap").c_str());
}

extern "C" {

const char* ddamg_hip_last_error(void) { return g_ddamg_last_error.c_str(); }

void ddamg_hip_default_params(ddamg_hip_params* p) {
  // reference defaults: src/init.c:778-812 (per level), :833-868 (general), :946-953 (k-cycle)
  memset(p, 0, sizeof *p);
  p->num_levels = 2;
  for (int i = 0; i < DDAMG_HIP_MAX_LEVELS; i++) {
    for (int mu = 0; mu < 4; mu++) { p->local_lattice[i][mu] = 0; p->block_lattice[i][mu] = 0; }
    p->num_vect[i] = 20;
    p->post_smooth_iter[i] = 2;
    p->block_iter[i] = 4;
    p->setup_iter[i] = (i == 0) ? 6 : (i == 1 ? 3 : 2);
  }
  p->restart = 10; p->max_restart = 100; p->tol = 1e-10;
  p->coarse_iter = 25; p->coarse_restart = 40; p->coarse_tol = 5e-2;
  p->kcycle = 1; p->kcycle_restart = 5; p->kcycle_max_restart = 2; p->kcycle_tol = 1e-1;
  p->mixed_precision = 2; p->odd_even = 1; p->method = 2;
  p->m0 = 0; p->csw = 0; p->device = 0;
  for (int mu = 0; mu < 4; mu++) { p->process_grid[mu] = 1; p->process_coords[mu] = 0; }
  p->test_vector_rng = 0; p->rng_seed = 0; p->gather_coarsest = 0;
}

int ddamg_hip_create(const ddamg_hip_params* p, ddamg_hip_ctx** out) {
  DDAMG_API_BEGIN
  const Knobs knobs = Knobs::from_env();   // the one read of the environment for this context
  DDAMG_REQUIRE(p && out, "null argument");
  DDAMG_REQUIRE(p->num_levels >= 1 && p->num_levels <= DDAMG_HIP_MAX_LEVELS, "1 <= num_levels <= 4");
  // the reference asserts -1 <= method <= 5 itself (src/init.c:982): its method-6 code (g5D_*) cannot be selected
  DDAMG_REQUIRE(p->method >= -1 && p->method <= 5, "method must be -1 (CGN), 0 (GMRES), 1/2/3 (additive / red-black / sixteen-colour SAP), 4 (GMRES smoother) "
                                                   "or 5 (FGMRES + BiCGstab, no AMG); the reference accepts no other value either (src/init.c:982)");
  DDAMG_REQUIRE(p->method != 5 || p->mixed_precision != 2, "method 5 runs with mixed_precision 0 or 1 (ASSERT( g.mixed_precision != 2 ), src/preconditioner.c:66)");
  DDAMG_REQUIRE(p->method != 5 || p->odd_even == 1, "method 5 is implemented on the odd-even Schur complement (odd_even = 1)");
  DDAMG_REQUIRE(p->mixed_precision >= 0 && p->mixed_precision <= 2, "mixed_precision must be 0, 1 or 2");
  int ndev = 0;
  DDAMG_HIP_CHECK(hipGetDeviceCount(&ndev));
  DDAMG_REQUIRE(ndev > 0, "no HIP device visible: the MI355X path has no CPU fallback");
  DDAMG_REQUIRE(p->device >= 0 && p->device < ndev, "device ordinal out of range");
  DDAMG_HIP_CHECK(hipSetDevice(p->device));
  // the Krylov loops read one small result back per iteration: a host thread that spins on the completion signal sees it
  // ~15 us earlier than one that sleeps (2 % of a 32^4 solve); one process per GPU owns its core anyway, as the
  // reference's MPI ranks do.  Process-wide device flag.
  (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
  (void)hipGetLastError();
  std::unique_ptr<ddamg_hip_ctx> c(new ddamg_hip_ctx(knobs));
  c->par = *p;
  for (int mu = 0; mu < 4; mu++) if (c->par.process_grid[mu] < 1 && c->par.process_grid[mu] != -1) { c->par.process_grid[mu] = 1; c->par.process_coords[mu] = 0; }
  c->device = p->device;
  {
    bool grid = false;
    for (int mu = 0; mu < 4; mu++) grid = grid || p->process_grid[mu] > 1 || p->process_grid[mu] == -1;
    const int comm_cus = comm_cus_for(c->knobs, p->num_levels);
    if (grid && comm_cus > 0) DDAMG_HIP_CHECK(create_cu_masked_stream(&c->stream, comm_cus, false));
    else DDAMG_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  }
  DDAMG_HIP_CHECK(hipEventCreate(&c->ev0));
  DDAMG_HIP_CHECK(hipEventCreate(&c->ev1));
  for (int d = 0; d < p->num_levels; d++) {
    std::unique_ptr<Level> lv(new Level);
    lv->depth = d;
    lv->ndof = (d == 0) ? 12 : 2 * p->num_vect[d - 1];
    int A[4], B[4];
    for (int mu = 0; mu < 4; mu++) {
      const int L = p->local_lattice[d][mu];
      DDAMG_REQUIRE(L > 0, "local lattice extent must be positive");
      if (d + 1 < p->num_levels) {
        DDAMG_REQUIRE(p->local_lattice[d + 1][mu] > 0 && L % p->local_lattice[d + 1][mu] == 0,
                      "coarse lattice must divide the finer lattice");
        A[mu] = L / p->local_lattice[d + 1][mu];
        B[mu] = p->block_lattice[d][mu] > 0 ? p->block_lattice[d][mu] : A[mu];
      } else {
        A[mu] = L;
        B[mu] = L;  // coarsest level: one parity-ordered block (odd-even Schur complement solve)
      }
    }
    if (p->num_levels == 1) for (int mu = 0; mu < 4; mu++) {
      // single-level (pure Krylov / operator only): keep a Schwarz-friendly ordering if blocks are given
      if (p->block_lattice[0][mu] > 0 && p->local_lattice[0][mu] % p->block_lattice[0][mu] == 0) {
        B[mu] = p->block_lattice[0][mu];
        A[mu] = B[mu];
      }
    }
    lv->geom.build(p->local_lattice[d], B, A, c->par.process_grid, c->par.process_coords);
    lv->d_lex_of_site.alloc(lv->geom.V);
    DDAMG_HIP_CHECK(hipMemcpy(lv->d_lex_of_site, lv->geom.lex_of_site.data(), sizeof(int) * lv->geom.V, hipMemcpyHostToDevice));
    c->levels.push_back(std::move(lv));
  }
  const bool half[3] = {c->knobs.coarse_half, c->knobs.transfer_half, c->knobs.intermediate_half};   // by StorageKind
  for (int k = 0; k < 3; k++) if (half[k] && storage_refusal(c.get(), (StorageKind)k) == nullptr) c->storage.bits[k] = 16;
  srand(1000u * (unsigned)c->levels[0]->geom.rank);  // reference: srand( 1000*g.my_rank ) unless "randomize test vectors" (src/init.c:870-873)
  *out = c.release();
  DDAMG_API_END
}

int ddamg_hip_destroy(ddamg_hip_ctx* c) {
  DDAMG_API_BEGIN
  delete c;
  DDAMG_API_END
}

int ddamg_hip_memory_in_use(size_t* device_bytes, size_t* pinned_bytes) {
  if (device_bytes) *device_bytes = DeviceMemory::in_use.load();
  if (pinned_bytes) *pinned_bytes = PinnedMemory::in_use.load();
  return 0;
}

int ddamg_hip_link_reals(ddamg_hip_ctx* c, int* reals) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(reals, "null argument");
  DDAMG_REQUIRE(c->have_operator, "link_reals: no operator uploaded");
  *reals = c->fop32.link_reals();
  DDAMG_API_END
}

int ddamg_hip_set_coarse_storage(ddamg_hip_ctx* c, int bits) { return set_storage(c, Coarse, bits, "coarse"); }
int ddamg_hip_set_transfer_storage(ddamg_hip_ctx* c, int bits) { return set_storage(c, Transfer, bits, "transfer"); }
int ddamg_hip_set_intermediate_storage(ddamg_hip_ctx* c, int bits) { return set_storage(c, Intermediate, bits, "intermediate"); }

static void drop_clover_base(ddamg_hip_ctx* c) {
  if (c->clover_base) { (void)hipStreamSynchronize(c->stream); c->clover_base.reset(); }
  c->scale_even = c->scale_odd = 1.0;
}

// the coarse operators of a hierarchy that is set up, from the fine operator as it is now
static void rebuild_coarse_operators(ddamg_hip_ctx* c) {
  if (c->setup_done) for_each_mg(c, [](auto& mg) { mg.operator_changed(); mg.release_setup_workspace(); });
}

// what follows the upload of a new fine operator, from host arrays or from device arrays
static void operator_replaced(ddamg_hip_ctx* c) {
  c->have_operator = true;
  rebuild_coarse_operators(c);
}

static void upload_operator(ddamg_hip_ctx* c) {
  drop_clover_base(c);      // a new operator is unscaled
  const Geometry& g = c->levels[0]->geom;
  c->fop64.upload(g, c->D_host.data(), c->clover_host.data(), c->knobs, c->stream);
  c->fop32.upload(g, c->D_host.data(), c->clover_host.data(), c->knobs, c->stream);
  c->mirror_valid = true;
  c->from_links = false;    // ddamg_hip_set_gauge sets it behind this call
  operator_replaced(c);
}

// D_host / clover_host from the fp64 operator on the device when ddamg_hip_set_gauge*_device left them stale (of a scaled operator:
// the unscaled field, which is what they hold after ddamg_hip_set_gauge as well)
static void ensure_host_mirror(ddamg_hip_ctx* c) {
  if (c->mirror_valid) return;
  const size_t V = c->levels[0]->geom.V;
  DeviceBuffer<double> dD, dC;
  dD.alloc(72 * V);
  dC.alloc(84 * V);
  c->fop64.export_lex(dD, dC, c->clover_base ? c->clover_base.get() : nullptr, c->stream);
  c->D_host.resize(72 * V);
  c->clover_host.resize(84 * V);
  DDAMG_HIP_CHECK(hipMemcpyAsync(c->D_host.data(), dD, sizeof(double) * 72 * V, hipMemcpyDeviceToHost, c->stream));
  DDAMG_HIP_CHECK(hipMemcpyAsync(c->clover_host.data(), dC, sizeof(double) * 84 * V, hipMemcpyDeviceToHost, c->stream));
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->mirror_valid = true;
}

// links in device memory -> both fine operators, nothing through the host: what ddamg_hip_set_gauge_device / _set_gauge2_device
// and their _grid forms run on the caller's arrays and ddamg_hip_load_ildg_conf on its own.  On a process grid the neighbours'
// shell of links travels device to device over the transport (collective) and the plaquette is the global one.
static void links_to_operator(ddamg_hip_ctx* c, const double* hopp_dev, const double* clover_dev, int anti_pbc, double* plaquette, const char* name) {
  const Geometry& g = c->levels[0]->geom;
  DDAMG_REQUIRE(!g.distributed() || c->comm != nullptr, (std::string(name) + " on a process grid fetches the neighbours' links: install a transport first "
                                                         "(ddamg_hip_comm_init_rccl / ddamg_hip_comm_init_host / ddamg_hip_comm_init_mpi)").c_str());
  const size_t V = g.V;
  DeviceBuffer<double> dD, dC;   // the staging arrays of FineOp::upload, filled on the device
  dD.alloc(72 * V);
  dC.alloc(84 * V);
  const double pl = g.distributed()
                        ? gauge_to_operator_resident_grid(g, c->comm, hopp_dev, clover_dev, anti_pbc, c->par.m0, c->par.csw, dD, dC, c->stream)
                        : gauge_to_operator_resident(g.L, hopp_dev, clover_dev, anti_pbc, c->par.m0, c->par.csw, dD, dC, c->stream);
  if (plaquette) *plaquette = pl;
  drop_clover_base(c);      // a new operator is unscaled
  c->fop64.upload_staged(g, dD, dC, c->knobs, c->stream);
  c->fop32.upload_staged(g, dD, dC, c->knobs, c->stream);
  dD.reset(); dC.reset();
  c->fop64.init_halo(g); c->fop32.init_halo(g);
  c->mirror_valid = false;
  std::vector<double>().swap(c->D_host);
  std::vector<double>().swap(c->clover_host);
  c->from_links = hopp_dev == clover_dev;
  operator_replaced(c);
}

// grid: the _grid entry points, which take any context; the others refuse a process grid, where the call would be collective
static void set_gauge_resident(ddamg_hip_ctx* c, const double* hopp_dev, const double* clover_dev, int anti_pbc, double* plaquette, const char* name, bool grid) {
  enter(c);
  const Geometry& g = c->levels[0]->geom;
  DDAMG_REQUIRE(grid || !g.distributed(), (std::string(name) + ": this entry point takes links in device memory on a single process only, because the clover "
                                           "term on a process grid needs the neighbours' links: use ddamg_hip_set_gauge_device_grid / "
                                           "ddamg_hip_set_gauge2_device_grid there (collective; device to device), or ddamg_hip_set_gauge").c_str());
  const size_t V = g.V;
  ddamg_require_device_array(c, hopp_dev, sizeof(double) * 72 * V, name);
  if (clover_dev != hopp_dev) ddamg_require_device_array(c, clover_dev, sizeof(double) * 72 * V, name);
  links_to_operator(c, hopp_dev, clover_dev, anti_pbc, plaquette, name);
}

// gauge field -> operator fields in the reference's storage (dirac_setup, src/dirac.c:60-168), no upload
static double gauge_fields(ddamg_hip_ctx* c, const double* gauge_lex, int anti_pbc, double* D_out, double* clover_out) {
  const Geometry& g = c->levels[0]->geom;
  if (g.distributed()) {
    DDAMG_REQUIRE(c->comm != nullptr, "set_gauge on a process grid fetches the neighbours' links: install a transport first "
                                      "(ddamg_hip_comm_init_rccl / ddamg_hip_comm_init_host / ddamg_hip_comm_init_mpi)");
    return gauge_to_operator_dist(g, c->comm, gauge_lex, anti_pbc, c->par.m0, c->par.csw, D_out, clover_out, c->stream);
  }
  return gauge_to_operator_device(g.L, gauge_lex, anti_pbc, c->par.m0, c->par.csw, D_out, clover_out, c->stream);
}

int ddamg_hip_set_gauge2(ddamg_hip_ctx* c, const double* hopp_gauge_lex, const double* clover_gauge_lex, int anti_pbc, double* plaquette) {
  // D from the first field, clover term and plaquette from the second, ONE upload (and one rebuild of the hierarchy)
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(hopp_gauge_lex && clover_gauge_lex, "null argument");
  const Geometry& g = c->levels[0]->geom;
  c->D_host.resize((size_t)g.V * 72);
  c->clover_host.resize((size_t)g.V * 84);
  const bool two = hopp_gauge_lex != clover_gauge_lex;   // one field: both parts from one pass
  std::vector<double> D_unused(two ? (size_t)g.V * 72 : 0), cl_unused(two ? (size_t)g.V * 84 : 0);
  if (two) gauge_fields(c, hopp_gauge_lex, anti_pbc, c->D_host.data(), cl_unused.data());
  const double pl = gauge_fields(c, clover_gauge_lex, anti_pbc, two ? D_unused.data() : c->D_host.data(), c->clover_host.data());
  if (plaquette) *plaquette = pl;
  upload_operator(c);
  c->from_links = !two;
  DDAMG_API_END
}
int ddamg_hip_set_gauge(ddamg_hip_ctx* c, const double* gauge_lex, int anti_pbc, double* plaquette) { return ddamg_hip_set_gauge2(c, gauge_lex, gauge_lex, anti_pbc, plaquette); }

int ddamg_hip_set_gauge_device(ddamg_hip_ctx* c, const double* gauge_dev_lex, int anti_pbc, double* plaquette) {
  DDAMG_API_BEGIN
  set_gauge_resident(c, gauge_dev_lex, gauge_dev_lex, anti_pbc, plaquette, "ddamg_hip_set_gauge_device", false);
  DDAMG_API_END
}

int ddamg_hip_set_gauge2_device(ddamg_hip_ctx* c, const double* hopp_gauge_dev_lex, const double* clover_gauge_dev_lex, int anti_pbc, double* plaquette) {
  // D from the first field, clover term and plaquette from the second, one layout pass
  DDAMG_API_BEGIN
  set_gauge_resident(c, hopp_gauge_dev_lex, clover_gauge_dev_lex, anti_pbc, plaquette, "ddamg_hip_set_gauge2_device", false);
  DDAMG_API_END
}

int ddamg_hip_set_gauge_device_grid(ddamg_hip_ctx* c, const double* gauge_dev_lex, int anti_pbc, double* plaquette) {
  DDAMG_API_BEGIN
  set_gauge_resident(c, gauge_dev_lex, gauge_dev_lex, anti_pbc, plaquette, "ddamg_hip_set_gauge_device_grid", true);
  DDAMG_API_END
}

int ddamg_hip_set_gauge2_device_grid(ddamg_hip_ctx* c, const double* hopp_gauge_dev_lex, const double* clover_gauge_dev_lex, int anti_pbc, double* plaquette) {
  DDAMG_API_BEGIN
  set_gauge_resident(c, hopp_gauge_dev_lex, clover_gauge_dev_lex, anti_pbc, plaquette, "ddamg_hip_set_gauge2_device_grid", true);
  DDAMG_API_END
}

// ---- ILDG configurations ----
static void require_ildg_arrays(const ddamg_hip_ctx* c, const void* raw_dev, int precision, long long nsites, const double* links_dev, const char* name) {
  enter(c);
  DDAMG_REQUIRE(precision == 32 || precision == 64, (std::string(name) + ": precision must be 32 or 64").c_str());
  DDAMG_REQUIRE(nsites >= 0, (std::string(name) + ": negative number of sites").c_str());
  const size_t raw_bytes = (size_t)nsites * 72 * (precision / 8), link_bytes = (size_t)nsites * 72 * sizeof(double);
  ddamg_require_device_array(c, raw_dev, raw_bytes, name);
  ddamg_require_device_array(c, links_dev, link_bytes, name);
  DDAMG_REQUIRE((uintptr_t)raw_dev % (precision == 64 ? 16 : 8) == 0 && (uintptr_t)links_dev % 16 == 0,
                (std::string(name) + ": the arrays must be 16-byte aligned (fp32 file data: 8)").c_str());
  const char* a = (const char*)raw_dev; const char* b = (const char*)links_dev;
  DDAMG_REQUIRE(a + raw_bytes <= b || b + link_bytes <= a, (std::string(name) + ": the output and the input array overlap").c_str());
}

int ddamg_hip_ildg_to_links_device(ddamg_hip_ctx* c, const void* raw_dev, int precision, long long nsites, double* links_dev) {
  DDAMG_API_BEGIN
  require_ildg_arrays(c, raw_dev, precision, nsites, links_dev, "ddamg_hip_ildg_to_links_device");
  ildg_to_links(raw_dev, precision, (size_t)nsites, links_dev, c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_links_to_ildg_device(ddamg_hip_ctx* c, const double* links_dev, int precision, long long nsites, void* raw_dev) {
  DDAMG_API_BEGIN
  require_ildg_arrays(c, raw_dev, precision, nsites, links_dev, "ddamg_hip_links_to_ildg_device");
  links_to_ildg(links_dev, precision, (size_t)nsites, raw_dev, c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

namespace {
struct Event {   // one per staging chunk of ddamg_hip_load_ildg_conf
  hipEvent_t e = nullptr;
  Event() { DDAMG_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
  ~Event() { if (e) (void)hipEventDestroy(e); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
};
struct File {
  int fd;
  explicit File(const char* path) : fd(open(path, O_RDONLY)) {}
  ~File() { if (fd >= 0) close(fd); }
  File(const File&) = delete;
  File& operator=(const File&) = delete;
};
}  // namespace

// file -> pinned staging -> device: the record of `info` as links [V][4][9] complex fp64 in `links`.  The pread of chunk k + 1
// runs while the copy and the kernel of chunk k are on the stream; a pinned chunk is read into again once the copy out of it
// (its event) is done, the one raw chunk on the device is reused in stream order.  `part`: this process's part of the file's
// lattice (V = part.Vloc); on a process grid a chunk is gathered from the runs of L[3] sites that ddamg_hip_read_ildg_conf reads as
// rows, in its order, so that the chunk holds local lexicographic order.
static void ildg_record_to_links(ddamg_hip_ctx* c, const char* path, const struct ddamg_hip_lime_info& info, const ddamg_io::Part& part, double* links) {
  const size_t V = part.Vloc;
  const bool whole = part.Vloc == part.Vglob;
  const size_t site_bytes = (size_t)72 * (info.precision / 8);
  size_t chunk_sites = ((size_t)64 << 20) / site_bytes;
  if (c->knobs.ildg_chunk_sites.set && c->knobs.ildg_chunk_sites.value > 0) chunk_sites = (size_t)c->knobs.ildg_chunk_sites.value;
  if (chunk_sites > V) chunk_sites = V;
  File file(path);
  DDAMG_REQUIRE(file.fd >= 0, (std::string("cannot open LIME file '") + path + "'").c_str());
  PinnedBuffer<char> pinned[2];
  Event copied[2];
  DeviceBuffer<char> raw;
  pinned[0].alloc(chunk_sites * site_bytes);
  if (chunk_sites < V) pinned[1].alloc(chunk_sites * site_bytes);
  raw.alloc(chunk_sites * site_bytes);
  bool in_flight[2] = {false, false};
  size_t k = 0;
  try {
    for (size_t first = 0; first < V; first += chunk_sites, k++) {
      const size_t n = V - first < chunk_sites ? V - first : chunk_sites;
      const int b = (int)(k & 1);
      if (in_flight[b]) DDAMG_HIP_CHECK(hipEventSynchronize(copied[b].e));
      int rc = 0;
      if (whole) rc = ddamg_io::pread_all(file.fd, pinned[b].get(), n * site_bytes, (off_t)(info.data_offset + (long long)(first * site_bytes)));
      else
        for (size_t s = first; s < first + n && !rc;) {   // the pieces of rows inside this chunk
          const size_t row = s / part.L[3], x = s - row * part.L[3];
          const size_t len = std::min((size_t)part.L[3] - x, first + n - s);
          const size_t y = row % part.L[2], z = (row / part.L[2]) % part.L[1], t = row / ((size_t)part.L[2] * part.L[1]);
          const size_t gsite = (((part.O[0] + t) * part.G[1] + (part.O[1] + z)) * part.G[2] + (part.O[2] + y)) * part.G[3] + part.O[3] + x;
          rc = ddamg_io::pread_all(file.fd, pinned[b].get() + (s - first) * site_bytes, len * site_bytes, (off_t)(info.data_offset + (long long)(gsite * site_bytes)));
          s += len;
        }
      if (rc) throw std::runtime_error(std::string("LIME file '") + path + "' ends early");
      DDAMG_HIP_CHECK(hipMemcpyAsync(raw.get(), pinned[b].get(), n * site_bytes, hipMemcpyHostToDevice, c->stream));
      DDAMG_HIP_CHECK(hipEventRecord(copied[b].e, c->stream));
      in_flight[b] = true;
      ildg_to_links(raw.get(), info.precision, n, links + first * 72, c->stream);
    }
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);   // nothing of the staging may be in use when it is released
    throw;
  }
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
}

int ddamg_hip_load_ildg_conf(ddamg_hip_ctx* c, const char* path, int anti_pbc, double* plaquette_out, double* file_plaquette_out, int* has_file_plaquette_out) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(path, "null argument");
  const Geometry& g = c->levels[0]->geom;
  int G[4];
  for (int mu = 0; mu < 4; mu++) G[mu] = g.L[mu] * g.P[mu];
  // on a process grid: this process's part of the record, then the path that fetches the neighbours' links device to device
  DDAMG_REQUIRE(!g.distributed() || c->comm != nullptr, "ddamg_hip_load_ildg_conf on a process grid fetches the neighbours' links: install a transport first "
                                                        "(ddamg_hip_comm_init_rccl / ddamg_hip_comm_init_host / ddamg_hip_comm_init_mpi)");
  ddamg_io::Part part;
  DDAMG_REQUIRE(ddamg_io::make_part(G, g.P, g.pc, part) && part.Vloc == (size_t)g.V, "load_ildg_conf: the process grid does not divide the lattice");
  struct ddamg_hip_lime_info info;
  if (ddamg_io::ildg_checked_info(path, G, &info)) throw std::runtime_error(ddamg_hip_io_last_error());
  const double file_plaq = 3.0 * info.plaquette; const int has_plaq = info.has_plaquette;
  DeviceBuffer<double> links;
  links.alloc((size_t)g.V * 72);
  ildg_record_to_links(c, path, info, part, links);
  links_to_operator(c, links, links, anti_pbc, plaquette_out, "ddamg_hip_load_ildg_conf");
  if (file_plaquette_out) *file_plaquette_out = file_plaq;
  if (has_file_plaquette_out) *has_file_plaquette_out = has_plaq;
  DDAMG_API_END
}

int ddamg_hip_clover_kernel_time(ddamg_hip_ctx* c, const double* gauge_dev_lex, int which, int reps, float* milliseconds, double* plaquette) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(milliseconds, "null argument");
  const Geometry& g = c->levels[0]->geom;
  DDAMG_REQUIRE(which == 3 ? (g.distributed() && c->comm != nullptr) : !g.distributed(),
                "ddamg_hip_clover_kernel_time: which = 0, 1, 2 on a single process only; which = 3 (the field-strength kernel on the extended lattice) on "
                "a process grid with a transport only");
  ddamg_require_device_array(c, gauge_dev_lex, sizeof(double) * 72 * g.V, "ddamg_hip_clover_kernel_time");
  const double pl = which == 3 ? extended_field_strength_timed(g, c->comm, gauge_dev_lex, reps, c->ev0, c->ev1, c->stream, milliseconds)
                               : clover_kernels_timed(g.L, gauge_dev_lex, c->par.m0, c->par.csw, which, reps, c->ev0, c->ev1, c->stream, milliseconds);
  if (plaquette) *plaquette = pl;
  DDAMG_API_END
}

// shift_update (src/dirac.c:646-668): m0 -> new_m0 on the operator that is set, on the device: the clover diagonals of both
// precisions, the 6x6 inverses of the odd-even kernels, and the self couplings of every coarse level (+ their inverses).
// No upload, no Galerkin construction; the host copy handed out by dd_alpha_amg_get_clover_pointer follows.
int ddamg_hip_shift_mass(ddamg_hip_ctx* c, double new_m0) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->have_operator, "no operator set");
  DDAMG_REQUIRE(c->scale_even == 1.0 && c->scale_odd == 1.0, "shift_mass on a scaled operator: undo ddamg_hip_scale_clover first (scale 1, 1)");
  const double diff = new_m0 - c->par.m0;
  if (diff != 0.0) {
    drop_clover_base(c);
    const size_t V = c->levels[0]->geom.V;
    c->fop64.shift_diagonal(c->fop64.clover_field(), diff, c->stream);
    c->fop32.shift_diagonal(c->fop64.clover_field(), 0.0, c->stream);
    if (c->setup_done) for_each_mg(c, [&](auto& mg) { mg.mass_shifted(diff); });
    if (c->mirror_valid)   // a stale host copy stays stale: what rebuilds it reads the device fields shifted above
      for (size_t s = 0; s < V; s++)
        for (int k = 0; k < 12; k++) c->clover_host[(s * 42 + k) * 2] += diff;
    c->par.m0 = new_m0;
    DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  }
  DDAMG_API_END
}

// scale_clover + operator_updates (src/dirac.c:624-644, src/dirac_generic.c:465-501; dd_alpha_amg_wilson_solve scales the clover term
// around a solve, src/dd_alpha_amg.c:354-373): the clover term of both precisions times scale_even / scale_odd by global parity on
// the device, the 6x6 inverses rebuilt, the coarse operators rebuilt from the interpolation operators that are there.  No host
// loop, no upload.  (1, 1) restores the unscaled field bit for bit.  The host copy handed out by dd_alpha_amg_get_clover_pointer
// keeps the unscaled field, as the reference's does after its solve.
int ddamg_hip_scale_clover(ddamg_hip_ctx* c, double scale_even, double scale_odd) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->have_operator, "no operator set");
  if (scale_even == c->scale_even && scale_odd == c->scale_odd) return 0;
  const size_t bytes = sizeof(double) * 72 * (size_t)c->levels[0]->geom.V;
  if (!c->clover_base) {
    c->clover_base.alloc(bytes / sizeof(double));
    DDAMG_HIP_CHECK(hipMemcpyAsync(c->clover_base, c->fop64.clover_field(), bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  c->fop64.scale_clover(c->clover_base, scale_even, scale_odd, c->stream);
  c->fop32.scale_clover(c->clover_base, scale_even, scale_odd, c->stream);
  c->scale_even = scale_even; c->scale_odd = scale_odd;
  rebuild_coarse_operators(c);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (scale_even == 1.0 && scale_odd == 1.0) c->clover_base.reset();
  DDAMG_API_END
}

int ddamg_hip_set_operator(ddamg_hip_ctx* c, const double* D_lex, const double* clover_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(D_lex && clover_lex, "null argument");
  const Geometry& g = c->levels[0]->geom;
  if (D_lex != c->D_host.data()) c->D_host.assign(D_lex, D_lex + (size_t)g.V * 72);
  if (clover_lex != c->clover_host.data()) c->clover_host.assign(clover_lex, clover_lex + (size_t)g.V * 84);
  upload_operator(c);
  DDAMG_API_END
}

int ddamg_hip_rccl_unique_id(void* id128) {
  DDAMG_API_BEGIN
  DDAMG_REQUIRE(id128, "null argument");
  rccl_unique_id(id128);
  DDAMG_API_END
}

static void install_comm(ddamg_hip_ctx* c, Comm* comm) {
  if (c->comm) comm_destroy(c->comm);
  c->comm = comm;
  c->fop32.set_comm(comm);
  c->fop64.set_comm(comm);
  c->rw_outer.comm = comm; c->rw_blas.comm = comm; c->rw_mp.comm = comm;
  for_each_mg(c, [&](auto& mg) { mg.set_comm(comm); });
  // creating a communicator may draw from libc rand() inside the communication library (observed: the first RCCL
  // communicator of a process does); the reference's test vectors come from the stream seeded at init and touched by
  // nothing else (src/init.c:870-873), so restore that state
  srand(1000u * (unsigned)c->levels[0]->geom.rank);
}

int ddamg_hip_comm_init_rccl(ddamg_hip_ctx* c, const void* id128) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(id128, "null argument");
  install_comm(c, comm_create_rccl(c->levels[0]->geom, id128, comm_cus_for(c->knobs, c->par.num_levels)));
  DDAMG_API_END
}

int ddamg_hip_comm_init_host(ddamg_hip_ctx* c, ddamg_hip_exchange_fn fn, ddamg_hip_allreduce_fn reduce_fn, void* user) {
  DDAMG_API_BEGIN
  enter(c);
  install_comm(c, comm_create_host(c->levels[0]->geom, fn, reduce_fn, user, comm_cus_for(c->knobs, c->par.num_levels)));
  DDAMG_API_END
}

const char* ddamg_hip_comm_stats(ddamg_hip_ctx* c, int reset) {
  if (!c || !c->comm) return "{}";
  if (reset) { comm_stats_reset(c->comm); return "{}"; }
  return comm_stats_json(c->comm);
}

int ddamg_hip_halo_plan(const int local_lattice[4], const int process_grid[4], const int process_coords[4],
                        int face, int* neighbor_rank, int* count, int* lex_sites) {
  DDAMG_API_BEGIN
  DDAMG_REQUIRE(local_lattice && process_grid && process_coords, "null argument");
  DDAMG_REQUIRE(face >= 0 && face < 8, "face must be 0..7");
  Geometry g;
  g.build(local_lattice, local_lattice, local_lattice, process_grid, process_coords);
  if (neighbor_rank) *neighbor_rank = g.neighbor_rank[face];
  if (count) *count = (int)g.face_sites[face].size();
  if (lex_sites) for (size_t i = 0; i < g.face_sites[face].size(); i++) lex_sites[i] = g.lex_of_site[g.face_sites[face][i]];
  DDAMG_API_END
}

int ddamg_hip_get_operator(ddamg_hip_ctx* c, double* D_lex, double* clover_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->have_operator, "no operator set");
  ensure_host_mirror(c);
  if (D_lex) memcpy(D_lex, c->D_host.data(), sizeof(double) * c->D_host.size());
  if (clover_lex) memcpy(clover_lex, c->clover_host.data(), sizeof(double) * c->clover_host.size());
  DDAMG_API_END
}

int ddamg_hip_vec_create(ddamg_hip_ctx* c, int level, int precision, ddamg_hip_vec** out) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(out, "null argument");
  DDAMG_REQUIRE(level >= 0 && level < (int)c->levels.size(), "level out of range");
  DDAMG_REQUIRE(precision == 32 || precision == 64, "precision must be 32 or 64");
  std::unique_ptr<ddamg_hip_vec> v(new ddamg_hip_vec);
  v->level = level; v->precision = precision;
  v->ndof = c->levels[level]->ndof;
  v->V = c->levels[level]->geom.V;
  v->aos = level > 0 ? 1 : 0;
  v->data.alloc((size_t)v->V * v->ndof * 2 * (precision / 8));
  DDAMG_HIP_CHECK(hipMemsetAsync(v->data.get(), 0, v->data.bytes(), c->stream));
  *out = v.release();
  DDAMG_API_END
}

int ddamg_hip_vec_destroy(ddamg_hip_ctx* c, ddamg_hip_vec* v) {
  DDAMG_API_BEGIN
  if (!v) return 0;   // as free(NULL)
  enter(c);
  (void)hipStreamSynchronize(c->stream);
  delete v;
  DDAMG_API_END
}

// fp64 numbers in lattice order in device memory -> the vector in its layout and precision, and back
static void vec_from_lex_any(ddamg_hip_ctx* c, ddamg_hip_vec* v, const double* src_dev) {
  const int* tab = c->levels[v->level]->d_lex_of_site;
  with_vec(v, [&](auto* p) {
    if (v->aos) aos_from_lex(p, src_dev, tab, v->V, v->ndof, c->stream);
    else vec_from_lex(p, src_dev, tab, v->V, v->ndof, c->stream);
  });
}
static void vec_to_lex_any(ddamg_hip_ctx* c, const ddamg_hip_vec* v, double* dst_dev) {
  const int* tab = c->levels[v->level]->d_lex_of_site;
  with_vec(v, [&](const auto* p) {
    if (v->aos) aos_to_lex(dst_dev, p, tab, v->V, v->ndof, c->stream);
    else vec_to_lex(dst_dev, p, tab, v->V, v->ndof, c->stream);
  });
}

int ddamg_hip_vec_upload(ddamg_hip_ctx* c, ddamg_hip_vec* v, const double* host_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(v && host_lex, "null argument");
  const size_t nb = sizeof(double) * vec_len(v);
  double* st = c->stage(nb);
  DDAMG_HIP_CHECK(hipMemcpyAsync(st, host_lex, nb, hipMemcpyHostToDevice, c->stream));
  vec_from_lex_any(c, v, st);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_vec_download(ddamg_hip_ctx* c, const ddamg_hip_vec* v, double* host_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(v && host_lex, "null argument");
  const size_t nb = sizeof(double) * vec_len(v);
  double* st = c->stage(nb);
  vec_to_lex_any(c, v, st);
  DDAMG_HIP_CHECK(hipMemcpyAsync(host_lex, st, nb, hipMemcpyDeviceToHost, c->stream));
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_vec_upload_device(ddamg_hip_ctx* c, ddamg_hip_vec* v, const double* dev_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(v, "null argument");
  ddamg_require_device_array(c, dev_lex, sizeof(double) * vec_len(v), "ddamg_hip_vec_upload_device");
  vec_from_lex_any(c, v, dev_lex);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_vec_download_device(ddamg_hip_ctx* c, const ddamg_hip_vec* v, double* dev_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(v, "null argument");
  ddamg_require_device_array(c, dev_lex, sizeof(double) * vec_len(v), "ddamg_hip_vec_download_device");
  vec_to_lex_any(c, v, dev_lex);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_dirac_apply(ddamg_hip_ctx* c, ddamg_hip_vec* out, const ddamg_hip_vec* in) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(out && in, "null argument");
  DDAMG_REQUIRE(c->have_operator, "no operator set (call ddamg_hip_set_gauge / ddamg_hip_set_operator)");
  DDAMG_REQUIRE(out->level == 0 && in->level == 0, "fine-level vectors expected");
  DDAMG_REQUIRE(out->precision == in->precision, "precision mismatch");
  DDAMG_REQUIRE(out->data.get() != in->data.get(), "in-place apply is not supported");
  if (in->precision == 32) c->fop32.apply(vec_data<float>(out), vec_data<float>(in), c->stream);
  else c->fop64.apply(vec_data<double>(out), vec_data<double>(in), c->stream);
  DDAMG_API_END
}

int ddamg_hip_dirac_apply_dagger(ddamg_hip_ctx* c, ddamg_hip_vec* out, const ddamg_hip_vec* in) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(out && in, "null argument");
  DDAMG_REQUIRE(c->have_operator, "no operator set (call ddamg_hip_set_gauge / ddamg_hip_set_operator)");
  DDAMG_REQUIRE(out->level == 0 && in->level == 0, "fine-level vectors expected");
  DDAMG_REQUIRE(out->precision == in->precision, "precision mismatch");
  DDAMG_REQUIRE(out->data.get() != in->data.get(), "in-place apply is not supported");
  if (in->precision == 32) c->fop32.apply_dagger(vec_data<float>(out), vec_data<float>(in), c->stream);
  else c->fop64.apply_dagger(vec_data<double>(out), vec_data<double>(in), c->stream);
  DDAMG_API_END
}

int ddamg_hip_gamma5(ddamg_hip_ctx* c, ddamg_hip_vec* out, const ddamg_hip_vec* in) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(out && in, "null argument");
  DDAMG_REQUIRE(out->level == 0 && in->level == 0, "fine-level vectors expected");
  DDAMG_REQUIRE(out->precision == in->precision, "precision mismatch");
  with_vec(out, [&](auto* d) { using T = pointee<decltype(d)>; vec_gamma5<T>(d, vec_data<T>(in), whole(vec_len(out)), c->stream); });
  DDAMG_API_END
}

// ---- the even-odd preconditioned system: half fields, the Schur complement, log det of the clover blocks (eo_system.h) ----
// what the half-field and Schur entry points ask of a vector: fine level; the parity table comes with the first operator
static void require_eo_vec(const ddamg_hip_ctx* c, const ddamg_hip_vec* v, const char* name) {
  DDAMG_REQUIRE(v, "null argument");
  DDAMG_REQUIRE(v->level == 0, (std::string(name) + ": fine-level vectors expected").c_str());
  require_even_extents(c, name);
  DDAMG_REQUIRE(c->have_operator, (std::string(name) + ": no operator set (call ddamg_hip_set_gauge / ddamg_hip_set_operator)").c_str());
}
static void require_parity(int parity, const char* name) {
  DDAMG_REQUIRE(parity == 0 || parity == 1, (std::string(name) + ": parity must be 0 (even) or 1 (odd)").c_str());
}

int ddamg_hip_vec_upload_parity_device(ddamg_hip_ctx* c, ddamg_hip_vec* v, int parity, const double* half_dev, int zero_other) {
  DDAMG_API_BEGIN
  enter(c);
  require_eo_vec(c, v, "ddamg_hip_vec_upload_parity_device");
  require_parity(parity, "ddamg_hip_vec_upload_parity_device");
  ddamg_require_device_array(c, half_dev, sizeof(double) * vec_len(v) / 2, "ddamg_hip_vec_upload_parity_device");
  with_vec(v, [&](auto* p) {
    vec_from_half(p, half_dev, c->levels[0]->d_lex_of_site.get(), c->fop64.dev().parity, parity, zero_other != 0, false, v->V, c->stream);
  });
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_vec_download_parity_device(ddamg_hip_ctx* c, const ddamg_hip_vec* v, int parity, double* half_dev) {
  DDAMG_API_BEGIN
  enter(c);
  require_eo_vec(c, v, "ddamg_hip_vec_download_parity_device");
  require_parity(parity, "ddamg_hip_vec_download_parity_device");
  ddamg_require_device_array(c, half_dev, sizeof(double) * vec_len(v) / 2, "ddamg_hip_vec_download_parity_device");
  with_vec(v, [&](const auto* p) {
    vec_to_half(half_dev, p, c->levels[0]->d_lex_of_site.get(), c->fop64.dev().parity, parity, false, v->V, c->stream);
  });
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_schur_apply(ddamg_hip_ctx* c, ddamg_hip_vec* out, const ddamg_hip_vec* in, int dagger) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(out && in, "null argument");
  require_eo_vec(c, out, "ddamg_hip_schur_apply");
  require_eo_vec(c, in, "ddamg_hip_schur_apply");
  DDAMG_REQUIRE(out->precision == in->precision, "precision mismatch");
  DDAMG_REQUIRE(out->data.get() != in->data.get(), "in-place apply is not supported");
  if (in->precision == 32) schur_apply<float>(c->fop32, vec_data<float>(out), vec_data<float>(in), dagger != 0, c->eo, c->stream);
  else schur_apply<double>(c->fop64, vec_data<double>(out), vec_data<double>(in), dagger != 0, c->eo, c->stream);
  DDAMG_API_END
}

int ddamg_hip_schur_apply_device(ddamg_hip_ctx* c, double* out_e_dev, const double* in_e_dev, int dagger) {
  DDAMG_API_BEGIN
  enter(c);
  const char* name = "ddamg_hip_schur_apply_device";
  require_even_extents(c, name);
  DDAMG_REQUIRE(c->have_operator, "no operator set (call ddamg_hip_set_gauge / ddamg_hip_set_operator)");
  const int V = c->levels[0]->geom.V;
  const size_t nb = sizeof(double) * 12 * V;
  ddamg_require_device_array(c, out_e_dev, nb, name);
  ddamg_require_device_array(c, in_e_dev, nb, name);
  ddamg_require_disjoint(out_e_dev, in_e_dev, nb, name);
  DeviceBuffer<double> in, out;     // full-length vectors for this call only
  in.alloc((size_t)24 * V);
  out.alloc((size_t)24 * V);
  const int* lex = c->levels[0]->d_lex_of_site.get();
  const unsigned char* par = c->fop64.dev().parity;
  vec_from_half<double>(in, in_e_dev, lex, par, 0, true, false, V, c->stream);
  schur_apply<double>(c->fop64, out, in, dagger != 0, c->eo, c->stream);
  vec_to_half<double>(out_e_dev, out, lex, par, 0, false, V, c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_schur_odd_part_device(ddamg_hip_ctx* c, int dagger, double* x_o_dev, const double* x_e_dev) {
  DDAMG_API_BEGIN
  enter(c);
  const char* name = "ddamg_hip_schur_odd_part_device";
  require_even_extents(c, name);
  DDAMG_REQUIRE(c->have_operator, "no operator set (call ddamg_hip_set_gauge / ddamg_hip_set_operator)");
  const int V = c->levels[0]->geom.V;
  const size_t nb = sizeof(double) * 12 * V;
  ddamg_require_device_array(c, x_o_dev, nb, name);
  ddamg_require_device_array(c, x_e_dev, nb, name);
  ddamg_require_disjoint(x_o_dev, x_e_dev, nb, name);
  DeviceBuffer<double> X;     // a full-length vector for this call only
  X.alloc((size_t)24 * V);
  const int* lex = c->levels[0]->d_lex_of_site.get();
  const unsigned char* par = c->fop64.dev().parity;
  vec_from_half<double>(X, x_e_dev, lex, par, 0, true, false, V, c->stream);
  // as solve_schur_core ends: X_o = -D_oo^-1 D_oe x_e (dagger: -gamma5 D_oo^-1 D_oe gamma5 x_e)
  const double* t = schur_odd_part<double>(c->fop64, X, dagger != 0, c->eo, c->stream);
  parity_update<double>(X, t, par, 1, ParityOp::MinusAssign, dagger != 0, V, c->stream);
  vec_to_half<double>(x_o_dev, X, lex, par, 1, false, V, c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_multishift_update_time(ddamg_hip_ctx* c, int nshift, int nactive, int reps, float* milliseconds) {
  DDAMG_API_BEGIN
  enter(c);
  const char* name = "ddamg_hip_multishift_update_time";
  DDAMG_REQUIRE(milliseconds, "null argument");
  require_even_extents(c, name);
  DDAMG_REQUIRE(nshift >= 1 && nshift <= DDAMG_HIP_MAX_SHIFTS && nactive >= 0 && nactive < nshift && reps >= 1,
                "ddamg_hip_multishift_update_time: 1 <= nshift <= DDAMG_HIP_MAX_SHIFTS, 0 <= nactive < nshift (the base system comes on top), reps >= 1");
  const Geometry& g = c->levels[0]->geom;
  const size_t n = (size_t)24 * g.V, half = n / 2;
  multishift_prepare(c->ms, g.parity, c->stream);
  ReduceWork& rw = c->ms.rw;
  DeviceBuffer<double> p, r, slab;
  p.alloc(n); r.alloc(n); slab.alloc(2 * (size_t)nshift * half);
  vec_random<double>(p, n, 11, 0, c->stream);
  vec_random<double>(r, n, 11, 1, c->stream);
  vec_random<double>(slab, 2 * (size_t)nshift * half, 11, 2, c->stream);
  // coefficients under which every field stays bounded over any number of launches: slot 0 is the base system, the last
  // `nactive` slots are the active shifts
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));   // no upload of an earlier solve still reads h_coef
  double* hc = rw.h_coef;
  hc[0] = nactive; hc[1] = 0.5; hc[2] = 0.0; hc[3] = 0.0;
  for (int a = 0; a < nactive; a++) {
    double* e = hc + MS_COEF_HEAD + MS_COEF_PER * a;
    e[0] = nshift - nactive + a; e[1] = 0.0; e[2] = 0.5; e[3] = 0.25;
  }
  upload_coefficients(rw, MS_COEF_HEAD + MS_COEF_PER * nactive, c->stream);
  auto launch = [&] { multishift_update(p, r, slab, slab + (size_t)nshift * half, rw.d_coef, c->ms.even_site.get(), g.V, c->stream); };
  launch();
  DDAMG_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
  for (int i = 0; i < reps; i++) launch();
  DDAMG_HIP_CHECK(hipEventRecord(c->ev1, c->stream));
  DDAMG_HIP_CHECK(hipEventSynchronize(c->ev1));
  float ms = 0;
  DDAMG_HIP_CHECK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *milliseconds = ms / reps;
  DDAMG_API_END
}

int ddamg_hip_clover_logdet(ddamg_hip_ctx* c, int parity, double* log_abs_det, int* sign) {
  DDAMG_API_BEGIN
  enter(c);
  const char* name = "ddamg_hip_clover_logdet";
  DDAMG_REQUIRE(log_abs_det && sign, "null argument");
  require_parity(parity, name);
  require_even_extents(c, name);
  DDAMG_REQUIRE(c->have_operator, "no operator set (call ddamg_hip_set_gauge / ddamg_hip_set_operator)");
  DDAMG_REQUIRE(!c->levels[0]->geom.distributed() || c->comm != nullptr, "ddamg_hip_clover_logdet on a process grid sums over the processes: install a transport first");
  ReduceWork& rw = blas_rw(c);
  clover_logdet(c->fop64.clover_field(), c->fop64.dev().parity, parity, c->levels[0]->geom.V, rw, rw.d_result, c->stream);
  publish_to_host(rw.d_result, 3, rw, c->stream);
  wait_published(rw, c->stream);
  DDAMG_REQUIRE(rw.h_result[2] == 0.0, parity ? "ddamg_hip_clover_logdet: a clover block on the odd sites (parity 1) is singular: zero or non-finite pivot"
                                              : "ddamg_hip_clover_logdet: a clover block on the even sites (parity 0) is singular: zero or non-finite pivot");
  *log_abs_det = rw.h_result[0];
  *sign = ((long long)rw.h_result[1] & 1) ? -1 : 1;
  DDAMG_API_END
}

// ---- the fermion force: derivatives of the operator that is set with respect to its links (force.h) ----
// what every force entry point asks of the context and of the output array, which must lie apart from [in, in + in_bytes) of each input.
// grid: the collective _grid entry points, which take any context; the others refuse a process grid.  Everything here is checked
// before the first message of a collective call.
static void require_force(const ddamg_hip_ctx* c, const double* force_dev, const char* name, bool grid) {
  const Geometry& g = c->levels[0]->geom;
  DDAMG_REQUIRE(grid || !g.distributed(), (std::string(name) + ": on a process grid the force needs the neighbours' shell of the links and of the site "
                                           "tensor and their face of the vectors, so the call is collective there; this non-collective form is not built "
                                           "yet for a process grid: use " + name + "_grid there (every process calls it, with a transport installed)").c_str());
  DDAMG_REQUIRE(!g.distributed() || c->comm != nullptr, (std::string(name) + " on a process grid fetches the neighbours' shell: install a transport first "
                                                         "(ddamg_hip_comm_init_rccl / ddamg_hip_comm_init_host / ddamg_hip_comm_init_mpi)").c_str());
  DDAMG_REQUIRE(c->have_operator, (std::string(name) + ": no operator set (call ddamg_hip_set_gauge / ddamg_hip_set_gauge_device)").c_str());
  DDAMG_REQUIRE(c->from_links, (std::string(name) + ": the operator did not come from one link field (ddamg_hip_set_operator and the two-field "
                                "ddamg_hip_set_gauge2* forms have none behind them): set it with ddamg_hip_set_gauge* / ddamg_hip_load_ildg_conf").c_str());
  ddamg_require_device_array(c, force_dev, sizeof(double) * 72 * g.V, name);
}
static void require_force_apart(const double* force_dev, const void* in, size_t in_bytes, size_t V, const char* name) {
  const char* a = (const char*)force_dev; const char* b = (const char*)in;
  DDAMG_REQUIRE(a + sizeof(double) * 72 * V <= b || b + in_bytes <= a, (std::string(name) + ": the output and the input array overlap").c_str());
}
static void force_bilinear_any(ddamg_hip_ctx* c, double* force_dev, const double* y, const double* x, double coeff, int accumulate) {
  const Geometry& g = c->levels[0]->geom;
  if (g.distributed())
    force_bilinear_grid(c->fop64, g, c->comm, c->levels[0]->d_lex_of_site.get(), c->par.csw, c->scale_even, c->scale_odd, y, x, coeff, accumulate, force_dev,
                        c->force, c->stream);
  else
    force_bilinear(c->fop64, g.L, c->levels[0]->d_lex_of_site.get(), c->par.csw, c->scale_even, c->scale_odd, y, x, coeff, accumulate, force_dev, c->force,
                   c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (g.distributed()) comm_release_device_staging(c->comm);     // the pinned staging of the host transport
}

static void force_bilinear_vec_any(ddamg_hip_ctx* c, double* force_dev, const ddamg_hip_vec* y, const ddamg_hip_vec* x, double coeff, int accumulate,
                                   const char* name, bool grid) {
  enter(c);
  DDAMG_REQUIRE(y && x, "null argument");
  DDAMG_REQUIRE(y->level == 0 && x->level == 0, (std::string(name) + ": fine-level vectors expected").c_str());
  DDAMG_REQUIRE(y->precision == 64 && x->precision == 64, (std::string(name) + ": the force is computed in fp64: fp32 vectors are refused").c_str());
  require_force(c, force_dev, name, grid);
  require_force_apart(force_dev, y->data.get(), y->data.bytes(), y->V, name);
  require_force_apart(force_dev, x->data.get(), x->data.bytes(), x->V, name);
  force_bilinear_any(c, force_dev, vec_data<double>(y), vec_data<double>(x), coeff, accumulate);
}
int ddamg_hip_force_bilinear_vec(ddamg_hip_ctx* c, double* force_dev, const ddamg_hip_vec* y, const ddamg_hip_vec* x, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_bilinear_vec_any(c, force_dev, y, x, coeff, accumulate, "ddamg_hip_force_bilinear_vec", false);
  DDAMG_API_END
}
int ddamg_hip_force_bilinear_vec_grid(ddamg_hip_ctx* c, double* force_dev, const ddamg_hip_vec* y, const ddamg_hip_vec* x, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_bilinear_vec_any(c, force_dev, y, x, coeff, accumulate, "ddamg_hip_force_bilinear_vec_grid", true);
  DDAMG_API_END
}

static void force_bilinear_device_any(ddamg_hip_ctx* c, double* force_dev, const double* y_dev, const double* x_dev, double coeff, int accumulate,
                                      const char* name, bool grid) {
  enter(c);
  require_force(c, force_dev, name, grid);
  const int V = c->levels[0]->geom.V;
  const size_t nb = sizeof(double) * 24 * V;
  ddamg_require_device_array(c, y_dev, nb, name);
  ddamg_require_device_array(c, x_dev, nb, name);
  require_force_apart(force_dev, y_dev, nb, V, name);
  require_force_apart(force_dev, x_dev, nb, V, name);
  if (!c->force.x.get()) { c->force.x.alloc((size_t)24 * V); c->force.y.alloc((size_t)24 * V); }
  const int* lex = c->levels[0]->d_lex_of_site.get();
  vec_from_lex<double>(c->force.y, y_dev, lex, V, 12, c->stream);
  vec_from_lex<double>(c->force.x, x_dev, lex, V, 12, c->stream);
  force_bilinear_any(c, force_dev, c->force.y, c->force.x, coeff, accumulate);
}
int ddamg_hip_force_bilinear_device(ddamg_hip_ctx* c, double* force_dev, const double* y_dev, const double* x_dev, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_bilinear_device_any(c, force_dev, y_dev, x_dev, coeff, accumulate, "ddamg_hip_force_bilinear_device", false);
  DDAMG_API_END
}
int ddamg_hip_force_bilinear_device_grid(ddamg_hip_ctx* c, double* force_dev, const double* y_dev, const double* x_dev, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_bilinear_device_any(c, force_dev, y_dev, x_dev, coeff, accumulate, "ddamg_hip_force_bilinear_device_grid", true);
  DDAMG_API_END
}

// ---- many pairs in one pass: force_dev (+)= coeff * sum_s weights[s] G(Y_s, X_s) (force.h: force_multi_*) ----
static_assert(DDAMG_HIP_FORCE_GROUP == force::GROUP, "include/ddamg_hip.h and force.h disagree on the pairs of a launch");
// the count, the arrays of pointers and the weights: what is checked before anything else is looked at
static void require_force_pairs(int n, const void* a, const void* b, const double* weights, const char* count, const char* name) {
  DDAMG_REQUIRE(n >= 1 && n <= DDAMG_HIP_MAX_FORCE_PAIRS,
                (std::string(name) + ": " + count + " = " + std::to_string(n) + " is outside 1 .. DDAMG_HIP_MAX_FORCE_PAIRS (32)").c_str());
  DDAMG_REQUIRE(a && b && weights, (std::string(name) + ": null argument (an array of pointers or the weights)").c_str());
  for (int s = 0; s < n; s++)
    DDAMG_REQUIRE(std::isfinite(weights[s]), (std::string(name) + ": weight " + std::to_string(s) + " is not finite").c_str());
}
// begin, the groups, end.  prepare(first, count, y, x): the vectors of the pairs first .. first + count - 1 in the operator's layout,
// which may live in c->force.group -- the stream orders a group's kernels before the next group's conversion
static void force_multi_run(ddamg_hip_ctx* c, double* force_dev, int n, const double* weights, double coeff, int accumulate,
                            const std::function<void(int, int, const double**, const double**)>& prepare) {
  const Geometry& g = c->levels[0]->geom;
  ForceMulti m = force_multi_begin(c->fop64, g, c->comm, c->levels[0]->d_lex_of_site.get(), c->par.csw, c->scale_even, c->scale_odd, c->force, c->stream);
  for (int first = 0; first < n; first += force::GROUP) {
    const int count = std::min((int)force::GROUP, n - first);
    const double* y[force::GROUP]; const double* x[force::GROUP];
    prepare(first, count, y, x);
    force_multi_group(m, g, c->comm, count, y, x, weights + first, c->force, c->stream);
  }
  force_multi_end(m, g, c->comm, coeff, accumulate, force_dev, c->force, c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (g.distributed()) comm_release_device_staging(c->comm);
}
// X then Y of pair k of a group in the workspace of 2 GROUP full vectors, in the context from the first call on
static double* force_group_vec(ddamg_hip_ctx* c, int k, bool is_y) {
  const size_t n = (size_t)24 * c->levels[0]->geom.V;
  if (!c->force.group.get()) c->force.group.alloc(2 * force::GROUP * n);
  DDAMG_REQUIRE(c->force.group.bytes() == sizeof(double) * 2 * force::GROUP * n, "force workspace of another lattice");
  return c->force.group.get() + (2 * (size_t)k + (is_y ? 1 : 0)) * n;
}

static void force_bilinear_multi_vec_any(ddamg_hip_ctx* c, double* force_dev, int npairs, const ddamg_hip_vec* const* y, const ddamg_hip_vec* const* x,
                                         const double* weights, double coeff, int accumulate, const char* name, bool grid) {
  enter(c);
  require_force_pairs(npairs, y, x, weights, "npairs", name);
  for (int s = 0; s < npairs; s++) {
    DDAMG_REQUIRE(y[s] && x[s], (std::string(name) + ": null argument (vector " + std::to_string(s) + ")").c_str());
    DDAMG_REQUIRE(y[s]->level == 0 && x[s]->level == 0, (std::string(name) + ": fine-level vectors expected").c_str());
    DDAMG_REQUIRE(y[s]->precision == 64 && x[s]->precision == 64, (std::string(name) + ": the force is computed in fp64: fp32 vectors are refused").c_str());
  }
  require_force(c, force_dev, name, grid);
  for (int s = 0; s < npairs; s++) {
    require_force_apart(force_dev, y[s]->data.get(), y[s]->data.bytes(), y[s]->V, name);
    require_force_apart(force_dev, x[s]->data.get(), x[s]->data.bytes(), x[s]->V, name);
  }
  force_multi_run(c, force_dev, npairs, weights, coeff, accumulate, [&](int first, int count, const double** yy, const double** xx) {
    for (int k = 0; k < count; k++) { yy[k] = vec_data<double>(y[first + k]); xx[k] = vec_data<double>(x[first + k]); }
  });
}
int ddamg_hip_force_bilinear_multi_vec(ddamg_hip_ctx* c, double* force_dev, int npairs, const ddamg_hip_vec* const* y, const ddamg_hip_vec* const* x,
                                       const double* weights, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_bilinear_multi_vec_any(c, force_dev, npairs, y, x, weights, coeff, accumulate, "ddamg_hip_force_bilinear_multi_vec", false);
  DDAMG_API_END
}
int ddamg_hip_force_bilinear_multi_vec_grid(ddamg_hip_ctx* c, double* force_dev, int npairs, const ddamg_hip_vec* const* y, const ddamg_hip_vec* const* x,
                                            const double* weights, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_bilinear_multi_vec_any(c, force_dev, npairs, y, x, weights, coeff, accumulate, "ddamg_hip_force_bilinear_multi_vec_grid", true);
  DDAMG_API_END
}

static void force_bilinear_multi_device_any(ddamg_hip_ctx* c, double* force_dev, int npairs, const double* const* y_dev, const double* const* x_dev,
                                            const double* weights, double coeff, int accumulate, const char* name, bool grid) {
  enter(c);
  require_force_pairs(npairs, y_dev, x_dev, weights, "npairs", name);
  for (int s = 0; s < npairs; s++)
    DDAMG_REQUIRE(y_dev[s] && x_dev[s], (std::string(name) + ": null argument (array " + std::to_string(s) + ")").c_str());
  require_force(c, force_dev, name, grid);
  const int V = c->levels[0]->geom.V;
  const size_t nb = sizeof(double) * 24 * V;
  for (int s = 0; s < npairs; s++) {
    ddamg_require_device_array(c, y_dev[s], nb, name);
    ddamg_require_device_array(c, x_dev[s], nb, name);
    require_force_apart(force_dev, y_dev[s], nb, V, name);
    require_force_apart(force_dev, x_dev[s], nb, V, name);
  }
  const int* lex = c->levels[0]->d_lex_of_site.get();
  force_multi_run(c, force_dev, npairs, weights, coeff, accumulate, [&](int first, int count, const double** yy, const double** xx) {
    for (int k = 0; k < count; k++) {
      double* X = force_group_vec(c, k, false); double* Y = force_group_vec(c, k, true);
      vec_from_lex<double>(Y, y_dev[first + k], lex, V, 12, c->stream);
      vec_from_lex<double>(X, x_dev[first + k], lex, V, 12, c->stream);
      yy[k] = Y; xx[k] = X;
    }
  });
}
int ddamg_hip_force_bilinear_multi_device(ddamg_hip_ctx* c, double* force_dev, int npairs, const double* const* y_dev, const double* const* x_dev,
                                          const double* weights, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_bilinear_multi_device_any(c, force_dev, npairs, y_dev, x_dev, weights, coeff, accumulate, "ddamg_hip_force_bilinear_multi_device", false);
  DDAMG_API_END
}
int ddamg_hip_force_bilinear_multi_device_grid(ddamg_hip_ctx* c, double* force_dev, int npairs, const double* const* y_dev, const double* const* x_dev,
                                               const double* weights, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_bilinear_multi_device_any(c, force_dev, npairs, y_dev, x_dev, weights, coeff, accumulate, "ddamg_hip_force_bilinear_multi_device_grid", true);
  DDAMG_API_END
}

// the rational force: X_s = (x_s, -D_oo^-1 D_oe x_s), Y_s = (Dhat x_s, -gamma5 D_oo^-1 D_oe gamma5 Dhat x_s), built group by group with
// the functions behind ddamg_hip_schur_apply_device, ddamg_hip_schur_odd_part_device and ddamg_hip_vec_upload_parity_device
static void force_rational_any(ddamg_hip_ctx* c, double* force_dev, int nshift, const double* rho, const double* const* x_e_dev,
                               const double* const* x_o_dev, double coeff, int accumulate, const char* name, bool grid) {
  enter(c);
  require_force_pairs(nshift, x_e_dev, x_e_dev, rho, "nshift", name);
  for (int s = 0; s < nshift; s++) DDAMG_REQUIRE(x_e_dev[s], (std::string(name) + ": null argument (x_e_dev[" + std::to_string(s) + "])").c_str());
  require_even_extents(c, name);
  require_force(c, force_dev, name, grid);
  const int V = c->levels[0]->geom.V;
  const size_t nb = sizeof(double) * 12 * V;
  for (int s = 0; s < nshift; s++) {
    ddamg_require_device_array(c, x_e_dev[s], nb, name);
    require_force_apart(force_dev, x_e_dev[s], nb, V, name);
    if (x_o_dev && x_o_dev[s]) {
      ddamg_require_device_array(c, x_o_dev[s], nb, name);
      require_force_apart(force_dev, x_o_dev[s], nb, V, name);
    }
  }
  const int* lex = c->levels[0]->d_lex_of_site.get();
  const unsigned char* par = c->fop64.dev().parity;
  force_multi_run(c, force_dev, nshift, rho, coeff, accumulate, [&](int first, int count, const double** yy, const double** xx) {
    for (int k = 0; k < count; k++) {
      const int s = first + k;
      double* X = force_group_vec(c, k, false); double* Y = force_group_vec(c, k, true);
      vec_from_half<double>(X, x_e_dev[s], lex, par, 0, true, false, V, c->stream);
      schur_apply<double>(c->fop64, Y, X, false, c->eo, c->stream);
      if (x_o_dev && x_o_dev[s]) {
        vec_from_half<double>(X, x_o_dev[s], lex, par, 1, false, false, V, c->stream);
      } else {
        const double* t = schur_odd_part<double>(c->fop64, X, false, c->eo, c->stream);
        parity_update<double>(X, t, par, 1, ParityOp::MinusAssign, false, V, c->stream);
      }
      const double* t = schur_odd_part<double>(c->fop64, Y, true, c->eo, c->stream);
      parity_update<double>(Y, t, par, 1, ParityOp::MinusAssign, true, V, c->stream);
      yy[k] = Y; xx[k] = X;
    }
  });
}
int ddamg_hip_force_rational_device(ddamg_hip_ctx* c, double* force_dev, int nshift, const double* rho, const double* const* x_e_dev,
                                    const double* const* x_o_dev, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_rational_any(c, force_dev, nshift, rho, x_e_dev, x_o_dev, coeff, accumulate, "ddamg_hip_force_rational_device", false);
  DDAMG_API_END
}
int ddamg_hip_force_rational_device_grid(ddamg_hip_ctx* c, double* force_dev, int nshift, const double* rho, const double* const* x_e_dev,
                                         const double* const* x_o_dev, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_rational_any(c, force_dev, nshift, rho, x_e_dev, x_o_dev, coeff, accumulate, "ddamg_hip_force_rational_device_grid", true);
  DDAMG_API_END
}

static void force_logdet_any(ddamg_hip_ctx* c, double* force_dev, int parity, double coeff, int accumulate, const char* name, bool grid) {
  enter(c);
  require_parity(parity, name);
  require_even_extents(c, name);
  require_force(c, force_dev, name, grid);
  // the pivot check of ddamg_hip_clover_logdet: the inverse blocks of a singular block are not a derivative of anything.  On a
  // process grid the flag is summed over the processes with the log det (sum_partials), so all of them refuse together, before
  // any shell is sent
  const Geometry& g = c->levels[0]->geom;
  ReduceWork& rw = blas_rw(c);
  clover_logdet(c->fop64.clover_field(), c->fop64.dev().parity, parity, g.V, rw, rw.d_result, c->stream);
  publish_to_host(rw.d_result, 3, rw, c->stream);
  wait_published(rw, c->stream);
  DDAMG_REQUIRE(rw.h_result[2] == 0.0, (std::string(name) + (parity ? ": a clover block on the odd sites (parity 1) is singular: zero or non-finite pivot"
                                                                      : ": a clover block on the even sites (parity 0) is singular: zero or non-finite pivot")).c_str());
  if (g.distributed())
    force_logdet_grid(c->fop64, g, c->comm, c->levels[0]->d_lex_of_site.get(), c->par.csw, c->scale_even, c->scale_odd, parity, coeff, accumulate, force_dev,
                      c->force, c->stream);
  else
    force_logdet(c->fop64, g.L, c->levels[0]->d_lex_of_site.get(), c->par.csw, c->scale_even, c->scale_odd, parity, coeff, accumulate, force_dev, c->force,
                 c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (g.distributed()) comm_release_device_staging(c->comm);
}
int ddamg_hip_force_logdet(ddamg_hip_ctx* c, double* force_dev, int parity, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_logdet_any(c, force_dev, parity, coeff, accumulate, "ddamg_hip_force_logdet", false);
  DDAMG_API_END
}
int ddamg_hip_force_logdet_grid(ddamg_hip_ctx* c, double* force_dev, int parity, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  force_logdet_any(c, force_dev, parity, coeff, accumulate, "ddamg_hip_force_logdet_grid", true);
  DDAMG_API_END
}

// ---- the gauge sector of the molecular dynamics (gauge_md.h): the context's lattice only, no operator ----
// the way into each of the twelve: the device, the refusal of a process grid by the plain forms (grid == false; the _grid twins take
// any context), and the sites of the local lattice.  `name` is the plain call's; name_of adds the suffix
static std::string name_of(const char* name, bool grid) { return std::string(name) + (grid ? "_grid" : ""); }
static size_t enter_gauge_md(const ddamg_hip_ctx* c, const char* name, bool grid) {
  enter(c);
  const Geometry& g = c->levels[0]->geom;
  DDAMG_REQUIRE(grid || !g.distributed(), (std::string(name) + ": refused on a process grid: the loops and the force need the neighbours' links (two sites deep "
                                           "with rectangles) and the sums run over all processes, so the call is collective there; this non-collective form "
                                           "is not built yet for a process grid: use " + name + "_grid there").c_str());
  return (size_t)g.V;
}
static void require_finite(double v, const char* what, const std::string& name) {
  DDAMG_REQUIRE(std::isfinite(v), (name + ": " + what + " is not finite").c_str());
}
// what a collective call of the gauge sector asks of a divided context, before the first message: a transport, and for the shell of
// the links (depth > 0) a local lattice at least as deep as the shell in every split direction
static void require_gauge_collective(const ddamg_hip_ctx* c, int depth, const std::string& name) {
  const Geometry& g = c->levels[0]->geom;
  DDAMG_REQUIRE(c->comm != nullptr, (name + " on a process grid is collective: install a transport first "
                                     "(ddamg_hip_comm_init_rccl / ddamg_hip_comm_init_host / ddamg_hip_comm_init_mpi)").c_str());
  for (int mu = 0; mu < 4; mu++)
    DDAMG_REQUIRE(!g.split[mu] || g.L[mu] >= depth,
                  (name + ": the local extent " + std::to_string(g.L[mu]) + " of the split direction " + std::to_string(mu) + " is below the depth " +
                   std::to_string(depth) + " of the shell of the links (2 with rectangles): the shell comes from one neighbour").c_str());
}

static void gauge_loops_any(ddamg_hip_ctx* c, const double* links_dev, double* plaquette_sum, double* rectangle_sum, const char* plain, bool grid) {
  const size_t V = enter_gauge_md(c, plain, grid);
  const std::string name = name_of(plain, grid);
  DDAMG_REQUIRE(plaquette_sum, "null argument");
  ddamg_require_device_array(c, links_dev, sizeof(double) * 72 * V, name.c_str());
  const Geometry& g = c->levels[0]->geom;
  if (!g.distributed()) {
    gauge_loops(g.L, links_dev, plaquette_sum, rectangle_sum, c->gauge_md, c->stream);
    return;
  }
  require_gauge_collective(c, gauge_depth(rectangle_sum != nullptr), name);
  double sums[2] = {0.0, 0.0};
  gauge_loops_grid(g, c->comm, links_dev, &sums[0], rectangle_sum ? &sums[1] : nullptr, c->gauge_md, c->stream);
  comm_release_device_staging(c->comm);
  comm_allreduce_host(c->comm, sums, rectangle_sum ? 2 : 1);
  *plaquette_sum = sums[0];
  if (rectangle_sum) *rectangle_sum = sums[1];
}
int ddamg_hip_gauge_loops_device(ddamg_hip_ctx* c, const double* links_dev, double* plaquette_sum, double* rectangle_sum) {
  DDAMG_API_BEGIN
  gauge_loops_any(c, links_dev, plaquette_sum, rectangle_sum, "ddamg_hip_gauge_loops_device", false);
  DDAMG_API_END
}
int ddamg_hip_gauge_loops_device_grid(ddamg_hip_ctx* c, const double* links_local_dev, double* plaquette_sum, double* rectangle_sum) {
  DDAMG_API_BEGIN
  gauge_loops_any(c, links_local_dev, plaquette_sum, rectangle_sum, "ddamg_hip_gauge_loops_device", true);
  DDAMG_API_END
}

static void gauge_force_any(ddamg_hip_ctx* c, double* force_dev, const double* links_dev, double beta, double c1, double coeff, int accumulate,
                            const char* plain, bool grid) {
  const size_t V = enter_gauge_md(c, plain, grid);
  const std::string name = name_of(plain, grid);
  ddamg_require_device_array(c, force_dev, sizeof(double) * 72 * V, name.c_str());
  ddamg_require_device_array(c, links_dev, sizeof(double) * 72 * V, name.c_str());
  ddamg_require_disjoint(force_dev, links_dev, sizeof(double) * 72 * V, name.c_str());
  require_finite(beta, "beta", name); require_finite(c1, "c1", name); require_finite(coeff, "coeff", name);
  const Geometry& g = c->levels[0]->geom;
  if (g.distributed()) require_gauge_collective(c, gauge_depth(c1 != 0.0), name);
  const size_t nslots = (size_t)4 * force::SLOTS * 9 * V;     // the plane slots of the fermion force: the same layout and size
  if (!c->force.slots.get()) c->force.slots.alloc(nslots);
  DDAMG_REQUIRE(c->force.slots.size() == nslots, "force workspace of another lattice");
  if (g.distributed()) gauge_force_grid(g, c->comm, links_dev, beta, c1, coeff, accumulate, force_dev, c->force.slots, c->gauge_md, c->stream);
  else gauge_force(g.L, links_dev, beta, c1, coeff, accumulate, force_dev, c->force.slots, c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (g.distributed()) comm_release_device_staging(c->comm);     // the pinned staging of the host transport
}
int ddamg_hip_gauge_force_device(ddamg_hip_ctx* c, double* force_dev, const double* links_dev, double beta, double c1, double coeff, int accumulate) {
  DDAMG_API_BEGIN
  gauge_force_any(c, force_dev, links_dev, beta, c1, coeff, accumulate, "ddamg_hip_gauge_force_device", false);
  DDAMG_API_END
}
int ddamg_hip_gauge_force_device_grid(ddamg_hip_ctx* c, double* force_local_dev, const double* links_local_dev, double beta, double c1, double coeff,
                                      int accumulate) {
  DDAMG_API_BEGIN
  gauge_force_any(c, force_local_dev, links_local_dev, beta, c1, coeff, accumulate, "ddamg_hip_gauge_force_device", true);
  DDAMG_API_END
}

// nothing is sent: on a grid the plain kernel on the local field
static void links_update_any(ddamg_hip_ctx* c, double* links_dev, const double* mom_dev, double eps, const char* plain, bool grid) {
  const size_t V = enter_gauge_md(c, plain, grid);
  const std::string name = name_of(plain, grid);
  ddamg_require_device_array(c, links_dev, sizeof(double) * 72 * V, name.c_str());
  ddamg_require_device_array(c, mom_dev, sizeof(double) * 72 * V, name.c_str());
  ddamg_require_disjoint(links_dev, mom_dev, sizeof(double) * 72 * V, name.c_str());
  require_finite(eps, "eps", name);
  links_update(V, links_dev, mom_dev, eps, c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
}
int ddamg_hip_links_update_device(ddamg_hip_ctx* c, double* links_dev, const double* mom_dev, double eps) {
  DDAMG_API_BEGIN
  links_update_any(c, links_dev, mom_dev, eps, "ddamg_hip_links_update_device", false);
  DDAMG_API_END
}
int ddamg_hip_links_update_device_grid(ddamg_hip_ctx* c, double* links_local_dev, const double* mom_local_dev, double eps) {
  DDAMG_API_BEGIN
  links_update_any(c, links_local_dev, mom_local_dev, eps, "ddamg_hip_links_update_device", true);
  DDAMG_API_END
}

// collective where the deviation is asked for.  The transports only sum, so the maximum travels as one slot per process in a zeroed
// array, summed, and is taken on the host; a NaN wins, as in the kernels
static void links_reunitarize_any(ddamg_hip_ctx* c, double* links_dev, double* max_deviation, const char* plain, bool grid) {
  const size_t V = enter_gauge_md(c, plain, grid);
  const std::string name = name_of(plain, grid);
  ddamg_require_device_array(c, links_dev, sizeof(double) * 72 * V, name.c_str());
  const bool collective = c->levels[0]->geom.distributed() && max_deviation;
  if (collective) require_gauge_collective(c, 0, name);
  links_reunitarize(V, links_dev, max_deviation, c->gauge_md, c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (collective) {
    std::vector<double> slot((size_t)comm_size(c->comm), 0.0);
    slot[(size_t)comm_rank(c->comm)] = *max_deviation;
    comm_allreduce_host(c->comm, slot.data(), (int)slot.size());
    double m = 0.0;
    for (double v : slot) m = (v > m || v != v) ? v : m;
    *max_deviation = m;
  }
}
int ddamg_hip_links_reunitarize_device(ddamg_hip_ctx* c, double* links_dev, double* max_deviation) {
  DDAMG_API_BEGIN
  links_reunitarize_any(c, links_dev, max_deviation, "ddamg_hip_links_reunitarize_device", false);
  DDAMG_API_END
}
int ddamg_hip_links_reunitarize_device_grid(ddamg_hip_ctx* c, double* links_local_dev, double* max_deviation) {
  DDAMG_API_BEGIN
  links_reunitarize_any(c, links_local_dev, max_deviation, "ddamg_hip_links_reunitarize_device", true);
  DDAMG_API_END
}

static void momentum_update_any(ddamg_hip_ctx* c, double* mom_dev, const double* force_dev, double eps, const char* plain, bool grid) {
  const size_t V = enter_gauge_md(c, plain, grid);
  const std::string name = name_of(plain, grid);
  ddamg_require_device_array(c, mom_dev, sizeof(double) * 72 * V, name.c_str());
  ddamg_require_device_array(c, force_dev, sizeof(double) * 72 * V, name.c_str());
  ddamg_require_disjoint(mom_dev, force_dev, sizeof(double) * 72 * V, name.c_str());
  require_finite(eps, "eps", name);
  momentum_update(V, mom_dev, force_dev, eps, c->stream);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
}
int ddamg_hip_momentum_update_device(ddamg_hip_ctx* c, double* mom_dev, const double* force_dev, double eps) {
  DDAMG_API_BEGIN
  momentum_update_any(c, mom_dev, force_dev, eps, "ddamg_hip_momentum_update_device", false);
  DDAMG_API_END
}
int ddamg_hip_momentum_update_device_grid(ddamg_hip_ctx* c, double* mom_local_dev, const double* force_local_dev, double eps) {
  DDAMG_API_BEGIN
  momentum_update_any(c, mom_local_dev, force_local_dev, eps, "ddamg_hip_momentum_update_device", true);
  DDAMG_API_END
}

// on a grid: this process's fixed-order sum, then the sum over the processes
static void momentum_kinetic_any(ddamg_hip_ctx* c, const double* mom_dev, double* kinetic, const char* plain, bool grid) {
  const size_t V = enter_gauge_md(c, plain, grid);
  const std::string name = name_of(plain, grid);
  DDAMG_REQUIRE(kinetic, "null argument");
  ddamg_require_device_array(c, mom_dev, sizeof(double) * 72 * V, name.c_str());
  const bool collective = c->levels[0]->geom.distributed();
  if (collective) require_gauge_collective(c, 0, name);
  double k = momentum_kinetic(V, mom_dev, c->gauge_md, c->stream);
  if (collective) comm_allreduce_host(c->comm, &k, 1);
  *kinetic = k;
}
int ddamg_hip_momentum_kinetic_device(ddamg_hip_ctx* c, const double* mom_dev, double* kinetic) {
  DDAMG_API_BEGIN
  momentum_kinetic_any(c, mom_dev, kinetic, "ddamg_hip_momentum_kinetic_device", false);
  DDAMG_API_END
}
int ddamg_hip_momentum_kinetic_device_grid(ddamg_hip_ctx* c, const double* mom_local_dev, double* kinetic) {
  DDAMG_API_BEGIN
  momentum_kinetic_any(c, mom_local_dev, kinetic, "ddamg_hip_momentum_kinetic_device", true);
  DDAMG_API_END
}

int ddamg_hip_get_site_order(ddamg_hip_ctx* c, int level, int* lex_of_site) {
  DDAMG_API_BEGIN
  DDAMG_REQUIRE(c, "null context");   // host tables only: no device is selected
  DDAMG_REQUIRE(lex_of_site, "null argument");
  DDAMG_REQUIRE(level >= 0 && level < (int)c->levels.size(), "level out of range");
  const Geometry& g = c->levels[level]->geom;
  for (int s = 0; s < g.V; s++) lex_of_site[s] = g.lex_of_site[s];
  DDAMG_API_END
}

int ddamg_hip_timer_begin(ddamg_hip_ctx* c) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
  DDAMG_API_END
}
int ddamg_hip_timer_end(ddamg_hip_ctx* c, float* ms) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(ms, "null argument");
  DDAMG_HIP_CHECK(hipEventRecord(c->ev1, c->stream));
  DDAMG_HIP_CHECK(hipEventSynchronize(c->ev1));
  DDAMG_HIP_CHECK(hipEventElapsedTime(ms, c->ev0, c->ev1));
  DDAMG_API_END
}
int ddamg_hip_sync(ddamg_hip_ctx* c) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

}  // extern "C"
