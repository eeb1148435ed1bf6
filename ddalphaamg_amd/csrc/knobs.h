// knobs.h -- every DDAMG_* environment switch of the library, read in ONE place.
//
// A context's switches are the environment at ddamg_hip_create: Knobs::from_env() runs there once, the result is a const
// member of the context, and everything created for that context is handed a reference to it.  Nothing below csrc/ calls
// getenv but this header.  The one exception to "per context" is DDAMG_POISON, which acts inside device_alloc where no
// context exists: it is read once per process (poison_allocations()).
//
// Standard library only (no HIP include): a host compiler builds this header alone (tests/test_knobs.py does).
#pragma once
#include <cstdlib>
#include <cstring>

namespace ddamg {

// an integer switch whose absence means something else than any of its values
struct OptionalInt {
  bool set = false;
  int value = 0;
};

struct Knobs {
  // ---- fine operator (FineOp<T>::upload) ----
  bool link_compression = true;     // DDAMG_LINK_COMPRESSION=0: full 18-real links instead of the two-row form
  bool link_pivot = true;           // DDAMG_LINK_PIVOT=0: the fp32 apply reads the two-row links instead of the 10-real pivot form
  bool clover_compression = true;   // DDAMG_CLOVER_COMPRESSION=0: the 72-real clover instead of the 56-real form of the fp32 apply

  // ---- ILDG configuration files (ddamg_hip_load_ildg_conf) ----
  OptionalInt ildg_chunk_sites;     // DDAMG_ILDG_CHUNK_SITES (tests): staging chunks of this many sites instead of 64 MiB of file data

  // ---- Schwarz smoother of the fine level (SapSmoother<T>::setup) ----
  // DDAMG_SAP_VARIANT  1: site-pair kernel, 2: thread-per-site kernel with resident operator, 3 (default): two blocks per
  // workgroup + face buffers where the shape allows (fp32, 4^4 blocks), else 2
  int sap_variant = 3;

  // ---- Galerkin construction of the first coarse operator (Multigrid<T>::build_coarse_operator) ----
  bool galerkin_unbatched = false;       // DDAMG_GALERKIN_UNBATCHED: column by column on both levels, not on the matrix cores
  bool galerkin_full_fields = false;     // DDAMG_GALERKIN_FULL_FIELDS: five full fields per column instead of the face-compacted ones
  bool galerkin_store_columns = false;   // DDAMG_GALERKIN_STORE_COLUMNS: the restriction through coarse column vectors and one store launch per column
  OptionalInt galerkin_slab_aggs;        // DDAMG_GALERKIN_SLAB_AGGS (tests): slabs of this many aggregates
  bool aggregate_dirac_gather = false;   // DDAMG_AGGREGATE_DIRAC_GATHER: the gather form of the compact field kernel instead of the tiled one
  bool coarse_restrict_valu = false;     // DDAMG_COARSE_RESTRICT_VALU: the coarse levels' restriction in its vector-unit form

  // ---- bootstrap of the setup (Multigrid<T>::bootstrap) ----
  bool bootstrap_unbatched = false;   // DDAMG_BOOTSTRAP_UNBATCHED: the fine level's V-cycles one vector at a time
  OptionalInt bootstrap_group;        // DDAMG_BOOTSTRAP_GROUP (tests): interpolation + smoothing in groups of this many vectors at any volume
  bool tv_gs_columnwise = false;      // DDAMG_TV_GS_COLUMNWISE: Gram-Schmidt on the test vectors column by column instead of by panels

  // ---- Gram-Schmidt on the aggregates ----
  bool gs_workgroup = false;               // DDAMG_GS_WORKGROUP: fine level, the workgroup form instead of one wavefront per aggregate and chirality
  bool coarse_gs_global = false;           // DDAMG_COARSE_GS_GLOBAL: coarse levels, the form that updates the vector through global memory
  bool coarse_gs_workgroup_form = false;   // DDAMG_COARSE_GS_FORM=w...: coarse levels, the bit-identical register form of one workgroup

  // ---- coarse operator ----
  bool coarse_sap_unfused = false;          // DDAMG_COARSE_SAP_UNFUSED: the coarse Schwarz block solver step by step instead of fused
  int coarse_apply_once_min_sites = 2048;   // DDAMG_COARSE_APPLY_ONCE_MIN_SITES: lattices from this size on read every link once (CoarseOp<T>::apply)
  bool coarse_half = false;                 // DDAMG_COARSE_HALF=1: a context starts with the coarsest couplings in 16-bit storage (ddamg_hip_set_coarse_storage)
  bool intermediate_half = false;           // DDAMG_INTERMEDIATE_HALF=1: a context starts with the intermediate levels' couplings in 16-bit storage (ddamg_hip_set_intermediate_storage)

  // ---- transfers of the fine level ----
  bool transfer_half = false;               // DDAMG_TRANSFER_HALF=1: a context starts with the fine level's interpolation operator in 16-bit storage (ddamg_hip_set_transfer_storage)

  // ---- Krylov solvers ----
  bool pipelined_arnoldi = false;          // DDAMG_PIPELINED_ARNOLDI: the reference's -DPIPELINED_ARNOLDI build, at run time (coarsest level)
  bool single_allreduce_arnoldi = false;   // DDAMG_SINGLE_ALLREDUCE_ARNOLDI: the reference's -DSINGLE_ALLREDUCE_ARNOLDI build, at run time (every GMRES)

  // ---- process grid ----
  OptionalInt comm_cus;          // DDAMG_COMM_CUS: compute units reserved for the transport stream (0: plain streams); see comm_cus_for
  bool host_transport = false;   // DDAMG_HIP_TRANSPORT=host: MPI moves staged buffers; default: RCCL over xGMI (dd_alpha_amg_* facade)

  // ---- diagnostics ----
  bool setup_timing = false;   // DDAMG_SETUP_TIMING: wall-clock seconds per setup phase on stderr

  static Knobs from_env() {
    const auto present = [](const char* name) { return getenv(name) != nullptr; };
    const auto unless_zero = [](const char* name) { const char* e = getenv(name); return !(e != nullptr && atoi(e) == 0); };
    const auto integer = [](const char* name) { const char* e = getenv(name); return e ? OptionalInt{true, atoi(e)} : OptionalInt{}; };
    Knobs k;
    k.link_compression = unless_zero("DDAMG_LINK_COMPRESSION");
    k.link_pivot = unless_zero("DDAMG_LINK_PIVOT");
    k.clover_compression = unless_zero("DDAMG_CLOVER_COMPRESSION");
    k.ildg_chunk_sites = integer("DDAMG_ILDG_CHUNK_SITES");
    if (const OptionalInt v = integer("DDAMG_SAP_VARIANT"); v.set) k.sap_variant = v.value;
    k.galerkin_unbatched = present("DDAMG_GALERKIN_UNBATCHED");
    k.galerkin_full_fields = present("DDAMG_GALERKIN_FULL_FIELDS");
    k.galerkin_store_columns = present("DDAMG_GALERKIN_STORE_COLUMNS");
    k.galerkin_slab_aggs = integer("DDAMG_GALERKIN_SLAB_AGGS");
    k.aggregate_dirac_gather = present("DDAMG_AGGREGATE_DIRAC_GATHER");
    k.coarse_restrict_valu = present("DDAMG_COARSE_RESTRICT_VALU");
    k.bootstrap_unbatched = present("DDAMG_BOOTSTRAP_UNBATCHED");
    k.bootstrap_group = integer("DDAMG_BOOTSTRAP_GROUP");
    k.tv_gs_columnwise = present("DDAMG_TV_GS_COLUMNWISE");
    k.gs_workgroup = present("DDAMG_GS_WORKGROUP");
    k.coarse_gs_global = present("DDAMG_COARSE_GS_GLOBAL");
    if (const char* e = getenv("DDAMG_COARSE_GS_FORM")) k.coarse_gs_workgroup_form = e[0] == 'w';
    k.coarse_sap_unfused = present("DDAMG_COARSE_SAP_UNFUSED");
    if (const OptionalInt v = integer("DDAMG_COARSE_APPLY_ONCE_MIN_SITES"); v.set) k.coarse_apply_once_min_sites = v.value;
    if (const OptionalInt v = integer("DDAMG_COARSE_HALF"); v.set) k.coarse_half = v.value != 0;
    if (const OptionalInt v = integer("DDAMG_INTERMEDIATE_HALF"); v.set) k.intermediate_half = v.value != 0;
    if (const OptionalInt v = integer("DDAMG_TRANSFER_HALF"); v.set) k.transfer_half = v.value != 0;
    k.pipelined_arnoldi = present("DDAMG_PIPELINED_ARNOLDI");
    k.single_allreduce_arnoldi = present("DDAMG_SINGLE_ALLREDUCE_ARNOLDI");
    k.comm_cus = integer("DDAMG_COMM_CUS");
    if (const char* e = getenv("DDAMG_HIP_TRANSPORT")) k.host_transport = strcmp(e, "host") == 0;
    k.setup_timing = present("DDAMG_SETUP_TIMING");
    return k;
  }
};

// compute units reserved for the transport stream of a context on a process grid: contexts without a hierarchy (operator,
// pure Krylov methods) reserve 24, multigrid contexts none; DDAMG_COMM_CUS overrides both (the measurements: common.h)
inline int comm_cus_for(const Knobs& knobs, int num_levels) { return knobs.comm_cus.set ? knobs.comm_cus.value : (num_levels <= 1 ? 24 : 0); }

// DDAMG_POISON: fill fresh device allocations with 0xFF bytes (device_alloc, device_buffer.h).  Per process, not per context.
inline bool poison_allocations() {
  static const bool on = getenv("DDAMG_POISON") != nullptr;
  return on;
}

}  // namespace ddamg
