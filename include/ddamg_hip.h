/*
 * ddamg_hip.h -- thin C-ABI of the MI355X (gfx950) implementation of the DDalphaAMG V-cycle hot path.
 *
 * This is the drop-in boundary *below* the reference's library interface (include/dd_alpha_amg.h):
 * plain pointers and sizes, no C++ / torch types.  Every entry point names the reference
 * interface it replaces (paths relative to the reference tree, mrottmann/DDalphaAMG).
 *
 * Conventions
 *  - directions / lattice extents are ordered T,Z,Y,X (reference src/clifford.h:33), X fastest;
 *  - host vectors are the reference's outer layout: lexicographic sites, `ndof` interleaved
 *    (re,im) double complex numbers per site (src/main_pre_def_generic.h:25-27,
 *    src/data_layout.h:30-32); ndof = 12 on the fine level, 2*num_vect on coarse levels;
 *  - every function returns 0 on success and a non-zero code on failure; the message is
 *    available from ddamg_hip_last_error().  (The reference aborts through error0/MPI_Abort,
 *    src/main.h:424-439; the dd_alpha_amg_* facade keeps that behaviour on top of these codes.)
 *  - one context per process and GPU; all work is enqueued on the context's HIP stream.
 */
#ifndef DDAMG_HIP_H
#define DDAMG_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDAMG_HIP_MAX_LEVELS 4

typedef struct ddamg_hip_ctx ddamg_hip_ctx;
typedef struct ddamg_hip_vec ddamg_hip_vec;
typedef struct ddamg_hip_chrono ddamg_hip_chrono;   /* a store of past solutions (ddamg_hip_chrono_create) */

/* Mirrors the parameters the reference reads from its .ini / dd_alpha_amg_parameters
 * (src/init.c:778-953, src/dd_alpha_amg_parameters.h:26-51).  Lattices in T,Z,Y,X order. */
typedef struct ddamg_hip_params {
  int num_levels;
  int local_lattice[DDAMG_HIP_MAX_LEVELS][4];
  int block_lattice[DDAMG_HIP_MAX_LEVELS][4];
  int num_vect[DDAMG_HIP_MAX_LEVELS];          /* "test vectors" per level                    */
  int post_smooth_iter[DDAMG_HIP_MAX_LEVELS];  /* Schwarz cycles per V-cycle                  */
  int block_iter[DDAMG_HIP_MAX_LEVELS];        /* MinRes steps per block solve                */
  int setup_iter[DDAMG_HIP_MAX_LEVELS];
  int restart, max_restart;                    /* outer FGMRES                                */
  double tol;
  int coarse_iter, coarse_restart;             /* coarsest-level GMRES                        */
  double coarse_tol;
  int kcycle, kcycle_restart, kcycle_max_restart;
  double kcycle_tol;
  int mixed_precision;                         /* 0: fp64 everywhere, 1: fp32 V-cycle / fp64 FGMRES, 2: fgmres_MP */
  int odd_even;
  int method;                                  /* -1 pure CGN, 0 pure GMRES; FGMRES + AMG with smoother 1 additive / 2 red-black / 3 sixteen-colour SAP, 4 GMRES; 5 FGMRES + BiCGstab without AMG (g.method, sample.ini) */
  double m0, csw;
  int device;                                  /* HIP device ordinal                          */
  /* domain decomposition over GPUs: one process per GPU on a Cartesian grid (reference: g.process_grid and
   * the MPI_Cart communicator, src/init.c:455-520 + src/data_layout.c:23-60).  rank = ((pt*Pz+pz)*Py+py)*Px+px.
   * local_lattice[] is the per-process lattice.  All 1 / 0: single GPU.  An entry of -1 means one process in that
   * direction whose +-mu faces nevertheless go through the transport (the process is its own neighbour): the complete
   * multi-GPU code path, RCCL included, on a single GPU -- for tests. */
  int process_grid[4];
  int process_coords[4];
  /* random test vectors of the setup: 0 = libc rand() consumed in the reference's order (src/data_generic.c:42-56;
   * reproduces the reference's hierarchies number for number, but costs ~5 ns per real on one host core),
   * 1 = counter-based generator on the device (the role of "randomize test vectors: 1", src/init.c:870-873) */
  int test_vector_rng;
  unsigned long long rng_seed;
  /* process grid only.  != 0: the coarsest level is not decomposed.  Every V-cycle gathers its right-hand side from all
   * processes (one all-gather over the transport), solves the coarsest system on the WHOLE coarsest lattice without any
   * communication, and keeps its own part of the solution.  This is the purpose of the reference's idle-process
   * gathering -- fewer, larger processes on the coarse levels, set there by a coarse "local lattice" larger than
   * global / process grid (src/init.c:56-72, vector_PRECISION_gather / _distribute src/gathering_generic.c:285-346) --
   * taken to its end point of ONE coarsest lattice; on GPUs every process solves it redundantly instead of all but one
   * idling, which also saves the distribute step.  The dd_alpha_amg_* facade sets it when the coarsest level's local lattice
   * equals its global lattice. */
  int gather_coarsest;
} ddamg_hip_params;

const char* ddamg_hip_last_error(void);

/* fills the reference's defaults (src/init.c:833-868,946-953) */
void ddamg_hip_default_params(ddamg_hip_params* p);

/* replaces method_init + operator_double_alloc/define (src/init.c:376-421) */
int ddamg_hip_create(const ddamg_hip_params* p, ddamg_hip_ctx** ctx);
/* replaces method_free + method_finalize (src/init.c:285-323,424-445) */
int ddamg_hip_destroy(ddamg_hip_ctx* ctx);

/* replaces dirac_setup (src/dirac.c:60-168): gauge links U [V][4][3x3 row-major complex] fp64,
 * lexicographic.  D = U/2, clover term from the four plaquette leaves, average plaquette returned.
 * anti_pbc != 0 negates the T-links of the last time slice first, as read_conf does
 * (src/io.c:536-541). */
int ddamg_hip_set_gauge(ddamg_hip_ctx* ctx, const double* gauge_lex, int anti_pbc, double* plaquette);
/* dirac_setup( hopp, clover ) with two different fields (src/dirac.c:60-168, as dd_alpha_amg_set_conf calls it for bc == 0,
 * src/dd_alpha_amg.c:205-246): the hopping term D = U/2 from `hopp_gauge_lex`, the clover term and the returned plaquette
 * from `clover_gauge_lex` (open boundaries: time links dropped from the hopping term near the boundary). */
int ddamg_hip_set_gauge2(ddamg_hip_ctx* ctx, const double* hopp_gauge_lex, const double* clover_gauge_lex, int anti_pbc, double* plaquette);

/* ---- fields that live in device memory ----------------------------------------------------------------------
 * Twins of the entry points that carry lattice data, for a host application that keeps its fields on the context's GPU (an
 * HMC or measurement code on the same card, a torch program).  The arrays have exactly the element order of their host twins
 * -- links [V][4][3x3 row-major complex] fp64, vectors [V][ndof] complex fp64, both lexicographic T,Z,Y,X with X fastest -- and
 * lie in the memory of the context's device.  Every device pointer is checked with hipPointerGetAttributes before anything is
 * launched: a null pointer, a host pointer, memory of another device or an allocation that is too small returns non-zero with a
 * message and leaves the context as it was.  Input arrays are never written; the output and the input array of one call must
 * not overlap.  The calls are synchronous towards the host, as their twins are: they return after the result is complete, and
 * the caller guarantees that whatever produced the input has finished (the context works on a stream of its own). */
/* ddamg_hip_set_gauge (dirac_setup, src/dirac.c:60-168) from links in device memory.  Nothing crosses PCIe: D = U/2 and the clover
 * term are computed into device staging arrays straight from the caller's links (the anti-periodic sign, which read_conf writes
 * into the links, src/io.c:536-541, is applied in the loads), the plaquette is summed on the device, and both precisions'
 * operators are laid out from the staging arrays.  Same effect on the context as ddamg_hip_set_gauge, except that the host copy
 * behind ddamg_hip_get_operator is not filled: it is rebuilt from the fp64 operator when it is asked for.  Refused, with a message
 * that names ddamg_hip_set_gauge_device_grid and ddamg_hip_set_gauge, on a context whose fine level is divided over processes
 * (process_grid entries > 1 or -1), because the clover term then needs the neighbours' links and the call becomes collective. */
int ddamg_hip_set_gauge_device(ddamg_hip_ctx* ctx, const double* gauge_dev_lex, int anti_pbc, double* plaquette);
/* ddamg_hip_set_gauge2 (dirac_setup( hopp, clover ), src/dirac.c:60-168) from two fields in device memory: D from the first, the
 * clover term and the plaquette from the second, one layout pass.  Equal pointers behave as ddamg_hip_set_gauge_device. */
int ddamg_hip_set_gauge2_device(ddamg_hip_ctx* ctx, const double* hopp_gauge_dev_lex, const double* clover_gauge_dev_lex, int anti_pbc, double* plaquette);
/* The same two on any process grid (the reference exchanges the ghost shell of the gauge field in dirac_setup, src/dirac.c:88-120).
 * Arguments and layout as above: this process's links [V][4][9] complex fp64, lexicographic T,Z,Y,X in the local lattice, never
 * written.  COLLECTIVE: every process of the grid calls it, with a transport installed (ddamg_hip_comm_init_rccl / _host / _mpi).
 * The links of the clover field are copied into the local lattice extended by one site in every split direction (the anti-periodic
 * sign goes in there, on the processes that hold the last global time slice), and the neighbours' shell, corners included, arrives
 * device to device: 72 doubles per shell site, two messages per split direction, one direction after the other; RCCL moves the
 * device buffers themselves, the host transport stages them through pinned memory.  The hopping field needs no shell.  The
 * extended array lives for the call only.  *plaquette is the global average (one all-reduce).  On a context that is not divided
 * they are ddamg_hip_set_gauge_device / _set_gauge2_device. */
int ddamg_hip_set_gauge_device_grid(ddamg_hip_ctx* ctx, const double* gauge_dev_lex, int anti_pbc, double* plaquette);
int ddamg_hip_set_gauge2_device_grid(ddamg_hip_ctx* ctx, const double* hopp_gauge_dev_lex, const double* clover_gauge_dev_lex, int anti_pbc, double* plaquette);
/* Milliseconds per launch of the kernels that turn links in device memory into the clover term, between the context's timer events
 * (as ddamg_hip_timer_begin / _end) after one untimed launch: which = 0 the field-strength kernel of ddamg_hip_set_gauge_device,
 * 1 the clover kernel of ddamg_hip_set_gauge, 2 the field-strength, assembly and plaquette-sum kernels together (0, 1, 2: single
 * process), 3 the field-strength kernel of ddamg_hip_set_gauge_device_grid on the extended lattice, which is built once before the
 * timed launches (a process grid with a transport; collective).  *plaquette: the average plaquette the kernels give (3: over this
 * process's sites).  The context is not changed.  For measurements (tools/device_interface_bench.py).  No
 * counterpart in the reference. */
int ddamg_hip_clover_kernel_time(ddamg_hip_ctx* ctx, const double* gauge_dev_lex, int which, int reps, float* milliseconds, double* plaquette);

/* ---- ILDG configurations (file format: ddamg_hip_io.h) ----------------------------------------------------------------
 * The raw data of an "ildg-binary-data" record in device memory -> links as ddamg_hip_set_gauge_device takes them, and back:
 * raw_dev holds nsites x 4 x 9 complex numbers, big-endian, fp64 (precision 64) or fp32 (32), directions X,Y,Z,T per site;
 * links_dev holds [nsites][4][9] complex fp64 in this library's order T,Z,Y,X.  One pass of a HIP kernel: byte order, direction
 * order and precision (fp32 widened exactly on the way in, rounded to nearest on the way out; fp64 bit patterns pass through
 * untouched).  For callers that read or write the record with their own parallel I/O; contract of "fields that live in device
 * memory" above; both arrays 16-byte aligned (fp32 raw data: 8).  Replaces the host loops byteswap8 + swap_spin_in_conf of
 * lime_read_conf (src/lime_io.c:50-72,273-314). */
int ddamg_hip_ildg_to_links_device(ddamg_hip_ctx* ctx, const void* raw_dev, int precision, long long nsites, double* links_dev);
int ddamg_hip_links_to_ildg_device(ddamg_hip_ctx* ctx, const double* links_dev, int precision, long long nsites, void* raw_dev);
/* lime_read_conf + dirac_setup (src/lime_io.c:222-337, src/dirac.c:60-168): the configuration of an ILDG file becomes the
 * operator.  Single process: the binary record is read in chunks (64 MiB of file data) into two pinned staging buffers, the read
 * of one chunk overlapping the copy and the conversion kernel of the one before, and the links land in a device array from which
 * the operator is built as ddamg_hip_set_gauge_device builds it; no host code touches a link.  On a process grid (collective, a
 * transport must be installed): each process reads its own part the same way -- a chunk is gathered from the runs of L[X] sites
 * that ddamg_hip_read_ildg_conf reads as rows -- and the operator is built as ddamg_hip_set_gauge_device_grid builds it.  The
 * file's lattice must be the context's global lattice.  *plaquette_out: the plaquette computed from the links, in [0,3];
 * *file_plaquette_out: three times the number of the file's "xlf-info" record if *has_file_plaquette_out (all three may be
 * NULL).  A failure leaves the operator that was set before in place. */
int ddamg_hip_load_ildg_conf(ddamg_hip_ctx* ctx, const char* path, int anti_pbc, double* plaquette_out, double* file_plaquette_out,
                             int* has_file_plaquette_out);

/* direct upload of an operator in the reference's own storage (g.op_double.D: [V][36] complex,
 * g.op_double.clover: [V][42] complex; src/dirac.c:80,386-398) -- the path behind
 * dd_alpha_amg_get_gauge_pointer / dd_alpha_amg_get_clover_pointer (src/dirac.c:171-176). */
int ddamg_hip_set_operator(ddamg_hip_ctx* ctx, const double* D_lex, const double* clover_lex);
/* shift_update (src/dirac.c:646-668): change the mass of the operator that is set, m0 -> new_m0, without a new upload and
 * without rebuilding the hierarchy: diagonal updates on the device on every level (shift_update_PRECISION
 * src/dirac_generic.c:504-551) and the inverses the odd-even kernels read.  ddamg_hip_get_operator shows the new clover field. */
int ddamg_hip_shift_mass(ddamg_hip_ctx* ctx, double new_m0);
/* scale_clover + operator_updates (src/dirac.c:624-644, src/dirac_generic.c:465-501), as dd_alpha_amg_wilson_solve applies them
 * around a solve (src/dd_alpha_amg.c:354-373): the clover term of every site times scale_even or scale_odd by the GLOBAL parity of
 * the site, on the device in both precisions, the 6x6 inverses of the odd-even kernels and the coarse operators following
 * (Galerkin construction with the interpolation operators that are there).  Scaling is absolute, not cumulative: (1, 1) restores
 * the unscaled operator bit for bit.  ddamg_hip_get_operator keeps showing the unscaled field. */
int ddamg_hip_scale_clover(ddamg_hip_ctx* ctx, double scale_even, double scale_odd);
/* read back the fp64 operator in the reference's storage (for parity tests) */
int ddamg_hip_get_operator(ddamg_hip_ctx* ctx, double* D_lex, double* clover_lex);

/* device vectors; precision is 32 or 64 */
int ddamg_hip_vec_create(ddamg_hip_ctx* ctx, int level, int precision, ddamg_hip_vec** v);
int ddamg_hip_vec_destroy(ddamg_hip_ctx* ctx, ddamg_hip_vec* v);
/* replaces trans_PRECISION / trans_back_PRECISION (src/schwarz_generic.c:1807-1846) */
int ddamg_hip_vec_upload(ddamg_hip_ctx* ctx, ddamg_hip_vec* v, const double* host_lex);
int ddamg_hip_vec_download(ddamg_hip_ctx* ctx, const ddamg_hip_vec* v, double* host_lex);

/* the same from / into an array in device memory (contract: "fields that live in device memory" above): trans_PRECISION /
 * trans_back_PRECISION (src/schwarz_generic.c:1807-1846) without the copy through the staging buffer */
int ddamg_hip_vec_upload_device(ddamg_hip_ctx* ctx, ddamg_hip_vec* v, const double* dev_lex);
int ddamg_hip_vec_download_device(ddamg_hip_ctx* ctx, const ddamg_hip_vec* v, double* dev_lex);

/* replaces d_plus_clover_float / d_plus_clover_double (src/dirac_generic.c:159-277) */
int ddamg_hip_dirac_apply(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in);
/* d_plus_clover_dagger_PRECISION (src/dirac_generic.c:281-285) in one pass: out = D^dagger in = gamma5 D gamma5 in, in the launches
 * of ddamg_hip_dirac_apply (the signs sit in the kernel's loads and in its store) and with the bits of the three passes.  Fine-level
 * vectors of equal precision, 32 or 64; out == in is refused, as by ddamg_hip_dirac_apply. */
int ddamg_hip_dirac_apply_dagger(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in);
/* gamma5_PRECISION (src/dirac_generic.c:288-297): spin components 0 and 1 change sign.  One launch; fine-level vectors of equal
 * precision, 32 or 64; out == in allowed */
int ddamg_hip_gamma5(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in);

/* BLAS-1 on device vectors: replaces vector_PRECISION_copy / vector_PRECISION_saxpy (z = x + alpha*y) and
 * global_inner_product_PRECISION <x,y> = sum conj(x_i) y_i together with global_norm_PRECISION(x)
 * (src/linalg_generic.c:29-353); reductions accumulate in fp64 */
int ddamg_hip_vec_copy(ddamg_hip_ctx* ctx, ddamg_hip_vec* dst, const ddamg_hip_vec* src);
int ddamg_hip_vec_axpy(ddamg_hip_ctx* ctx, ddamg_hip_vec* z, const ddamg_hip_vec* x, const ddamg_hip_vec* y, double alpha_re, double alpha_im);
int ddamg_hip_vec_dot(ddamg_hip_ctx* ctx, const ddamg_hip_vec* x, const ddamg_hip_vec* y, double* re, double* im, double* norm_x);

/* ---- multigrid hierarchy ------------------------------------------------------------------ */
/* replaces method_setup + method_update (src/init.c:134-374; dd_alpha_amg_setup, src/dd_alpha_amg.c:254-273):
 * random test vectors (libc rand(), as vector_PRECISION_define_random) -> smoother passes -> aggregate-wise
 * Gram-Schmidt -> Galerkin coarse operator, then `setup_iterations` bootstrap iterations
 * (inv_iter_inv_fcycle, src/setup_generic.c:441-503).  setup_iterations < 0: use params.setup_iter[0]. */
int ddamg_hip_setup(ddamg_hip_ctx* ctx, int setup_iterations, int* coarse_iterations);
/* the same with the iterative phase on the operator shifted to setup_m0 and back (method_setup at the solver mass, method_update at
 * g.setup_m0: src/init.c:134-374,326-357; dd_alpha_amg_par::setup_m0), in ONE lifetime of the setup workspace */
int ddamg_hip_setup_at_mass(ddamg_hip_ctx* ctx, int setup_iterations, double setup_m0, int* coarse_iterations);
/* replaces method_update / dd_alpha_amg_setup_update (src/dd_alpha_amg.c:288-310) */
int ddamg_hip_setup_update(ddamg_hip_ctx* ctx, int iterations, int* coarse_iterations);
/* replaces the "interpolation: 4" path (test vectors from outside, src/setup_generic.c:131-160 + re_setup :278-321):
 * tv_lex = [num_vect][V][12] complex fp64 lexicographic; orthonormalised != 0: the vectors are already
 * the aggregate-orthonormal interpolation vectors and are used as they are. */
int ddamg_hip_set_test_vectors(ddamg_hip_ctx* ctx, const double* tv_lex, int orthonormalised);
int ddamg_hip_get_interpolation(ddamg_hip_ctx* ctx, double* P_lex);
/* the level-0 test vectors themselves, same shape (what the reference writes for setup persistence: vector_io_single_file
 * "test vectors", src/io.c:951-1124; see ddamg_hip_io.h) */
int ddamg_hip_get_test_vectors(ddamg_hip_ctx* ctx, double* tv_lex);
/* coarse operator in the reference's storage, lexicographic coarse sites: D [Vc][4][n*n] complex as blocks
 * A,C,B,D column-major, clover [Vc][n(n+1)/2] complex packed (src/coarse_operator_generic.h:124-143,
 * src/coarse_operator_generic.c:109-111) */
int ddamg_hip_get_coarse_operator(ddamg_hip_ctx* ctx, double* D_lex, double* clover_lex);
int ddamg_hip_set_coarse_operator(ddamg_hip_ctx* ctx, const double* D_lex, const double* clover_lex);
/* the same for the operator of any coarse level 1 <= level < num_levels (l->next_level->...->op_PRECISION, built by
 * coarse_operator_PRECISION_setup src/coarse_operator_generic.c:53-100 on every level) */
int ddamg_hip_get_coarse_operator_level(ddamg_hip_ctx* ctx, int level, double* D_lex, double* clover_lex);
int ddamg_hip_set_coarse_operator_level(ddamg_hip_ctx* ctx, int level, const double* D_lex, const double* clover_lex);
/* interpolation vectors of level `level` < num_levels - 1 as they are (l->is_PRECISION.interpolation[] of that level after
 * gram_schmidt_on_aggregates, src/setup_generic.c:268-273): P_lex = [num_vect[level]][V_level][ndof_level] complex fp64,
 * lexicographic sites of that level.  Builds the operator of level + 1 from them (coarse_operator_PRECISION_setup) and
 * runs the initial setup of the levels below. */
int ddamg_hip_set_interpolation_level(ddamg_hip_ctx* ctx, int level, const double* P_lex);

/* ---- hot-path pieces, vectors in the V-cycle precision (32 unless mixed_precision == 0) ------ */
/* replaces smoother_PRECISION / red_black_schwarz_PRECISION (src/vcycle_generic.c:25-88,
 * src/schwarz_generic.c:1260-1431); initial_guess_zero != 0 is the reference's _NO_RES.  The vectors' level selects the
 * smoother (any level but the coarsest). */
int ddamg_hip_smoother(ddamg_hip_ctx* ctx, ddamg_hip_vec* phi, const ddamg_hip_vec* eta, int cycles, int initial_guess_zero);
/* replaces restrict_PRECISION / interpolate3_PRECISION (add == 0) / interpolate_PRECISION (add != 0)
 * (src/interpolation_generic.c:93-207) */
int ddamg_hip_restrict(ddamg_hip_ctx* ctx, ddamg_hip_vec* coarse, const ddamg_hip_vec* fine);
int ddamg_hip_interpolate(ddamg_hip_ctx* ctx, ddamg_hip_vec* fine, const ddamg_hip_vec* coarse, int add);
/* replaces apply_coarse_operator_PRECISION (src/coarse_operator_generic.c:383-394) */
int ddamg_hip_coarse_apply(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in);
/* The two products the coarsest odd-even Schur complement is made of (coarse_hopping_term / coarse_n_hopping_term and
 * coarse_diag_ee / coarse_diag_oo_inv, src/coarse_oddeven_generic.c:123-198, 447-729), on the sites of one parity of the coarsest
 * level (0: even, 1: odd; odd_even == 1), in the coarse storage that is set:
 *   hop:      out(x) = [accumulate ? out(x) : 0] + sign * (sum of the eight hopping terms of `in`)(x)    -- a "half hopping term"
 *   self_mul: out(x) = M0(x) in(x), or M0(x)^-1 in(x) with inverse != 0
 * The sites of the other parity in `out` are left as they are.  For measurements and kernel tests (tools/half_storage_bench.py). */
int ddamg_hip_coarse_hop(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in, int parity, double sign, int accumulate);
int ddamg_hip_coarse_self_mul(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in, int parity, int inverse);
/* replaces coarse_solve_odd_even_PRECISION (src/coarse_oddeven_generic.c:1139-1159) */
int ddamg_hip_coarse_solve(ddamg_hip_ctx* ctx, ddamg_hip_vec* x, const ddamg_hip_vec* b, int* iterations);
/* Storage of the coarsest level's couplings for the solve: bits = 32 (default) or 16.  With 16 the one-right-hand-side coarsest
 * odd-even solve (ddamg_hip_coarse_solve, and with it every V-cycle, K-cycle and ddamg_hip_solve) and ddamg_hip_coarse_apply on
 * coarsest-level vectors read a copy of the couplings and of the inverted self couplings that holds one fp16 pair (re, im) per
 * element and one fp32 scale per matrix; vectors and accumulation stay fp32.  The copy is made by its first use, follows every
 * change of the operator by itself (ddamg_hip_shift_mass, ddamg_hip_scale_clover, ddamg_hip_setup_update,
 * ddamg_hip_set_coarse_operator*), and is freed by setting 32 again.  ddamg_hip_setup, ddamg_hip_setup_at_mass and
 * ddamg_hip_setup_update always run on the 32-bit couplings: the hierarchy does not depend on the setting.  Callable at any time
 * after ddamg_hip_create; the initial value is 32, or 16 under DDAMG_COARSE_HALF=1 where the context can carry it.  Returns
 * non-zero, with the storage unchanged, if bits is neither 16 nor 32, and for 16 on a context without an fp32 multigrid hierarchy
 * (mixed_precision == 0, fewer than two levels, method 5), with odd_even == 0, or whose coarsest level is decomposed over
 * processes and not gathered (gather_coarsest).  No counterpart in the reference. */
int ddamg_hip_set_coarse_storage(ddamg_hip_ctx* ctx, int bits);
/* Storage of the fine level's interpolation operator P for the solve: bits = 32 (default) or 16.  With 16 ddamg_hip_restrict and
 * ddamg_hip_interpolate on fine-level vectors (and with them every V-cycle, K-cycle, ddamg_hip_preconditioner, ddamg_hip_solve
 * and ddamg_hip_solve_vec) read a copy of P that holds one fp16 number per real and one fp32 scale per aggregate, vector and
 * chirality; vectors and accumulation stay fp32.  The transfers of the intermediate levels stay fp32.  The copy costs half the
 * bytes of P again, is made by its first use, follows every change of P by itself (ddamg_hip_setup, ddamg_hip_setup_update,
 * ddamg_hip_set_test_vectors, ddamg_hip_set_interpolation), and is freed by setting 32 again.  ddamg_hip_setup,
 * ddamg_hip_setup_at_mass and ddamg_hip_setup_update always run on the 32-bit P: the hierarchy does not depend on the setting.
 * Callable at any time after ddamg_hip_create; the initial value is 32, or 16 under DDAMG_TRANSFER_HALF=1 where the context can
 * carry it.  Returns non-zero, with the storage unchanged, if bits is neither 16 nor 32, and for 16 on a context without an fp32
 * multigrid hierarchy (mixed_precision == 0, fewer than two levels, a method outside 1-4).  Process grids are not refused:
 * aggregates never cross a process boundary and the two kernels are local.  No counterpart in the reference. */
int ddamg_hip_set_transfer_storage(ddamg_hip_ctx* ctx, int bits);
/* Storage of the couplings of every intermediate level (depth > 0, not the coarsest) for the solve: bits = 32 (default) or 16.
 * With 16 the operator of those levels (ddamg_hip_coarse_apply on their vectors, the K-cycle's FGMRES), the residual updates of
 * their Schwarz smoother and its block solver (ddamg_hip_smoother on their vectors, and with them every V-cycle, K-cycle,
 * ddamg_hip_preconditioner, ddamg_hip_solve and ddamg_hip_solve_vec) read a copy of the couplings that holds one fp16 pair
 * (re, im) per element and one fp32 scale per matrix; vectors and accumulation stay fp32.  The many-vector paths of the
 * intermediate level and its transfers stay fp32.  There is one copy per intermediate level; each costs half the bytes of the
 * level's couplings again (about 3 GB at 64^4 with 16^4 x 48), is made by its first use, follows every change of the operator by
 * itself (ddamg_hip_shift_mass, ddamg_hip_scale_clover, ddamg_hip_setup_update, ddamg_hip_set_coarse_operator_level), and is
 * freed by setting 32 again.  ddamg_hip_setup, ddamg_hip_setup_at_mass and ddamg_hip_setup_update always run on the 32-bit
 * couplings: the hierarchy does not depend on the setting.  Callable at any time after ddamg_hip_create; the initial value is
 * 32, or 16 under DDAMG_INTERMEDIATE_HALF=1 where the context can carry it.  Returns non-zero, with the storage unchanged, if
 * bits is neither 16 nor 32, and for 16 on a context with fewer than three levels, with a method outside 1-3 (the GMRES smoother
 * of method 4 is not covered), with mixed_precision == 0, or with an intermediate level that is decomposed over processes.  No
 * counterpart in the reference. */
int ddamg_hip_set_intermediate_storage(ddamg_hip_ctx* ctx, int bits);
/* the same for ncols <= 32 right-hand sides at once: ncols independent GMRES recurrences advanced in lockstep, the coarse
 * operator applied to all columns on the matrix cores (v_mfma_f32_16x16x4_f32), as the bootstrap setup runs the coarsest-level
 * solves of its Nvec test vectors (the reference solves them one by one, src/setup_generic.c:441-503).  fp32 V-cycle, single
 * process, odd-even.  iterations[c]: GMRES iterations of column c, -1 if it needed more steps than the lockstep basis holds
 * (x[c] is then not written). */
int ddamg_hip_coarse_solve_many(ddamg_hip_ctx* ctx, int ncols, ddamg_hip_vec* const* x, const ddamg_hip_vec* const* b, int* iterations);
/* replaces vcycle_PRECISION(phi, NULL, eta, _NO_RES) (src/vcycle_generic.c:91-141) on the level of the vectors */
int ddamg_hip_vcycle(ddamg_hip_ctx* ctx, ddamg_hip_vec* phi, const ddamg_hip_vec* eta);
/* the K-cycle of an intermediate level: fgmres_PRECISION(&l->p_PRECISION) with the V-cycle of that level as preconditioner,
 * initial guess zero (src/vcycle_generic.c:110-114) */
int ddamg_hip_kcycle(ddamg_hip_ctx* ctx, ddamg_hip_vec* x, const ddamg_hip_vec* b, int* iterations);
/* Many right-hand sides (2 <= ncols <= 32) on a coarse level, as the bootstrap setup runs its Nvec independent V-cycles
 * (the reference: one test vector at a time, src/setup_generic.c:191-275,441-503): every coupling of a site becomes a complex
 * (n x n) x (n x 32) product on the matrix cores (v_mfma_f32_16x16x4_f32), the coupling matrices read once for all columns;
 * every column keeps its own MinRes coefficients, Hessenberg matrix and stopping test.  fp32 V-cycle, single process.
 * The level of the vectors selects the level: the intermediate level of three levels, or level 1 or 2 of four.
 *   coarse_apply_many: apply_coarse_operator_PRECISION on the coarsest level or on an intermediate level;
 *   smoother_many / vcycle_many / kcycle_many: red-black Schwarz smoother, V-cycle and K-cycle (iterations[c] per column) of
 *   an intermediate level.  On level 1 of four levels the V-cycle runs the K-cycles of level 2 for all columns inside it
 *   (vcycle_PRECISION -> fgmres_PRECISION(&l->next_level->p), src/vcycle_generic.c:103-114), every level with its own restart
 *   length, tolerance and smoother counts; that form needs kcycle = 1.
 * Non-zero, with the reason in ddamg_hip_last_error, for a null argument and where the many-vector path does not cover the
 * context (mixed_precision == 2, odd_even == 0, methods other than 2, process grids, more than 32 test vectors or 64 dof on
 * any intermediate level from the vectors' level down). */
int ddamg_hip_coarse_apply_many(ddamg_hip_ctx* ctx, int ncols, ddamg_hip_vec* const* out, const ddamg_hip_vec* const* in);
int ddamg_hip_smoother_many(ddamg_hip_ctx* ctx, int ncols, ddamg_hip_vec* const* phi, const ddamg_hip_vec* const* eta, int cycles, int initial_guess_zero);
int ddamg_hip_vcycle_many(ddamg_hip_ctx* ctx, int ncols, ddamg_hip_vec* const* phi, const ddamg_hip_vec* const* eta);
int ddamg_hip_kcycle_many(ddamg_hip_ctx* ctx, int ncols, ddamg_hip_vec* const* x, const ddamg_hip_vec* const* b, int* iterations);

/* replaces wilson_driver -> fgmres_double + preconditioner (src/top_level.c:64-104,
 * src/linsolve_generic.c:219-413): host vectors lexicographic fp64.  tol <= 0: params.tol.
 * relres = true relative residual ||b - D x|| / ||b|| recomputed in fp64 (FGMRES_RESTEST). */
int ddamg_hip_solve(ddamg_hip_ctx* ctx, double* x_lex, const double* b_lex, double tol,
                    int* iterations, int* coarse_iterations, double* relres);
/* the same solve on device-resident vectors (fine level, precision 64, filled with ddamg_hip_vec_upload, ddamg_hip_vec_upload_device
 * or by other device code): nothing crosses PCIe -- the form a GPU-resident host application uses */
int ddamg_hip_solve_vec(ddamg_hip_ctx* ctx, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol,
                        int* iterations, int* coarse_iterations, double* relres);
/* replaces preconditioner() (src/preconditioner.c:25-69): one V-cycle, fp64 lexicographic in/out */
int ddamg_hip_preconditioner(ddamg_hip_ctx* ctx, double* out_lex, const double* in_lex);
/* ddamg_hip_solve (wilson_driver -> fgmres_double + preconditioner, src/top_level.c:64-104) and ddamg_hip_preconditioner
 * (preconditioner(), src/preconditioner.c:25-69) on lexicographic fp64 arrays in device memory (contract: "fields that live in
 * device memory" above): the layout kernels read and write the caller's arrays, nothing crosses PCIe.  They work on process grids
 * as their twins do: the arrays are the process's own part. */
int ddamg_hip_solve_device(ddamg_hip_ctx* ctx, double* x_dev_lex, const double* b_dev_lex, double tol,
                           int* iterations, int* coarse_iterations, double* relres);
int ddamg_hip_preconditioner_device(ddamg_hip_ctx* ctx, double* out_dev_lex, const double* in_dev_lex);
/* D^dagger x = b through the hierarchy of D: x = gamma5 D^-1 gamma5 b.  The reference has the operator (d_plus_clover_dagger_PRECISION,
 * src/dirac_generic.c:281-285) and no driver for this solve.  gamma5 costs no pass over the vectors: the signs sit in the layout kernels
 * that load b and store x (in one gamma5 kernel each in place of the copies of the _vec form).  Every `method` and `mixed_precision` of
 * ddamg_hip_solve, and process grids (gamma5 is local).  relres, the iteration counts and ddamg_hip_residual_history are those of the
 * inner solve of D on gamma5 b; gamma5 changes signs only, so they are exactly the residuals of D^dagger x = b as well.  Arguments as
 * for ddamg_hip_solve, ddamg_hip_solve_vec and ddamg_hip_solve_device, refused alike. */
int ddamg_hip_solve_dagger(ddamg_hip_ctx* ctx, double* x_lex, const double* b_lex, double tol,
                           int* iterations, int* coarse_iterations, double* relres);
int ddamg_hip_solve_dagger_vec(ddamg_hip_ctx* ctx, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol,
                               int* iterations, int* coarse_iterations, double* relres);
int ddamg_hip_solve_dagger_device(ddamg_hip_ctx* ctx, double* x_dev_lex, const double* b_dev_lex, double tol,
                                  int* iterations, int* coarse_iterations, double* relres);
/* D^dagger D x = b (the pseudofermion heat-bath and force solves of an HMC; no counterpart in the reference):  y = D^-dagger b as above,
 * then x = D^-1 y; y never leaves the device and lives for the call only.  Both solves run to the same tol, each relative to its own
 * right-hand side.  iterations[0], coarse_iterations[0]: the D^dagger solve; [1]: the D solve (either array may be null).
 * relres = ||b - D^dagger D x|| / ||b||, recomputed in fp64 with the fp64 operator and its dagger: the residual of the system the
 * caller asked for.  It is NOT promised to be below tol: the error of the first solve passes through D^-1, so relres carries the
 * condition of D^dagger.  ddamg_hip_residual_history is that of the second solve. */
int ddamg_hip_solve_squared(ddamg_hip_ctx* ctx, double* x_lex, const double* b_lex, double tol,
                            int iterations[2], int coarse_iterations[2], double* relres);
int ddamg_hip_solve_squared_vec(ddamg_hip_ctx* ctx, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol,
                                int iterations[2], int coarse_iterations[2], double* relres);
int ddamg_hip_solve_squared_device(ddamg_hip_ctx* ctx, double* x_dev_lex, const double* b_dev_lex, double tol,
                                   int iterations[2], int coarse_iterations[2], double* relres);
enum { DDAMG_HIP_SYSTEM_D = 0, DDAMG_HIP_SYSTEM_DDAGGER = 1 };   /* `system` of the solves below */
/* A solve that starts from the caller's vector (no counterpart in the reference, whose interface starts every solve from zero): x
 * holds the guess x0 on entry and the solution on return.  system: DDAMG_HIP_SYSTEM_D solves D x = b, DDAMG_HIP_SYSTEM_DDAGGER solves
 * D^dagger x = b; with A that operator, the call forms r0 = b - A x0 with the fp64 operator, solves A e = r0 from zero by the solver of
 * ddamg_hip_solve (ddamg_hip_solve_dagger) to the tolerance tol ||b|| / ||r0||, and returns x = x0 + e: every `method`, every
 * `mixed_precision` and process grids.  tol <= 0: params.tol.  Where ||r0|| <= tol ||b|| already, x stays as it is and the counts are 0.
 * relres = ||b - A x|| / ||b|| recomputed in fp64 from the x that is returned: relative to b, not to r0.
 * guess_relres = ||r0|| / ||b||; both norms come out of one reduction, so a zero guess gives exactly 1 and the bits of the plain solve.
 * b = 0 gives x = 0, zero counts and zero residuals.  ddamg_hip_residual_history is that of the correction solve and so relative to
 * ||r0||, not to ||b||.  Arguments as for ddamg_hip_solve, ddamg_hip_solve_vec and ddamg_hip_solve_device, refused alike, as is a
 * system other than the two. */
int ddamg_hip_solve_guess(ddamg_hip_ctx* ctx, int system, double* x_lex, const double* b_lex, double tol,
                          int* iterations, int* coarse_iterations, double* relres, double* guess_relres);
int ddamg_hip_solve_guess_vec(ddamg_hip_ctx* ctx, int system, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol,
                              int* iterations, int* coarse_iterations, double* relres, double* guess_relres);
int ddamg_hip_solve_guess_device(ddamg_hip_ctx* ctx, int system, double* x_dev_lex, const double* b_dev_lex, double tol,
                                 int* iterations, int* coarse_iterations, double* relres, double* guess_relres);
/* A store of the last `depth` solutions (1 <= depth <= 8) and the chronological guess from them: the combination of the stored
 * vectors that minimises the residual of the system posed NOW (minimal residual extrapolation, Brower et al., Nucl. Phys. B 484
 * (1997) 353; no counterpart in the reference).  The solves of a molecular-dynamics trajectory, of a Hasenbusch chain or of a mass
 * scan are nearby systems: the operator may change between a push and a guess (ddamg_hip_shift_mass, ddamg_hip_set_gauge*), that is
 * the point.  The store owns depth fine fp64 vectors and, from its first guess on, the workspace of a guess (2 depth + 1 more); it
 * belongs to the context that created it, is refused by any other, and is destroyed before that context.
 *   create / destroy / reset (forget the vectors, keep the memory) / count (vectors held);  destroy with a null store is a no-op;
 *   push_vec: a ring, the oldest vector falls out;
 *   guess_vec: x0 = the guess for A x = b (system as above), kept = the vectors that entered it, predicted_relres = the residual
 *     ||b - A x0|| / ||b|| as the orthogonalisation predicts it (a prediction: the truth is guess_relres of the solve that follows).
 *     One fp64 operator application per stored vector, newest first; the images are orthonormalised by classical Gram-Schmidt applied
 *     twice with the same operations carried on the vectors -- the Gram matrix of the images is numerically singular exactly when the
 *     history is good, so no normal equations -- and a vector whose image loses all but 1e-12 of its norm in the projection (a
 *     duplicate) is left out.  An empty store gives x0 = 0, kept = 0 and predicted_relres = 1.
 *   solve_chrono_*: the guess, ddamg_hip_solve_guess from it, and the solution pushed.  x is output only.  Where the measured
 *     guess_relres is not finite or not below 1 the solve starts from zero instead and guess_relres is returned as 1.
 *   solve_squared_chrono_*: D^dagger D x = b as ddamg_hip_solve_squared, the D^dagger solve with the store hy (of the intermediate
 *     vectors y, which stay inside), the D solve with hx; either store may be null, which is a zero guess for that solve.  relres and
 *     the two pairs of counts as for ddamg_hip_solve_squared. */
int ddamg_hip_chrono_create(ddamg_hip_ctx* ctx, int depth, ddamg_hip_chrono** h);
int ddamg_hip_chrono_destroy(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h);
int ddamg_hip_chrono_reset(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h);
int ddamg_hip_chrono_count(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, int* n);
int ddamg_hip_chrono_push_vec(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, const ddamg_hip_vec* x);
int ddamg_hip_chrono_guess_vec(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, int system, ddamg_hip_vec* x0, const ddamg_hip_vec* b,
                               int* kept, double* predicted_relres);
int ddamg_hip_solve_chrono_vec(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, int system, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol,
                               int* iterations, int* coarse_iterations, double* relres, double* guess_relres);
int ddamg_hip_solve_chrono_device(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, int system, double* x_dev_lex, const double* b_dev_lex, double tol,
                                  int* iterations, int* coarse_iterations, double* relres, double* guess_relres);
int ddamg_hip_solve_squared_chrono_vec(ddamg_hip_ctx* ctx, ddamg_hip_chrono* hy, ddamg_hip_chrono* hx, ddamg_hip_vec* x, const ddamg_hip_vec* b,
                                       double tol, int iterations[2], int coarse_iterations[2], double* relres);
int ddamg_hip_solve_squared_chrono_device(ddamg_hip_ctx* ctx, ddamg_hip_chrono* hy, ddamg_hip_chrono* hx, double* x_dev_lex,
                                          const double* b_dev_lex, double tol, int iterations[2], int coarse_iterations[2], double* relres);
/* ---- the even-odd preconditioned system (no library interface in the reference, which has the operator:
 * apply_schur_complement_PRECISION, src/oddeven_generic.c:704-740) ---------------------------------------------------------
 * Conventions of everything in this group:
 *  - Parity.  The parity of a site is (t+z+y+x) mod 2 of its GLOBAL coordinates: 0 even, 1 odd.
 *  - Every call refuses, with a message, a context in which a local lattice extent is odd.  With even extents local and global
 *    parity agree, and every pair x = 2k, 2k+1 holds one site of each parity.
 *  - Half field.  [V/2][12] complex fp64: the sites of ONE parity of the process's own lattice in lexicographic order (T,Z,Y,X, X
 *    fastest); half index = lexicographic index >> 1.
 *  - Full-length vectors (fine-level ddamg_hip_vec) keep their layout: results are defined on the even sites and the odd sites
 *    hold zeros, unless stated otherwise below.
 *  - Systems.  Dhat = D_ee - D_eo D_oo^-1 D_oe on the even sites (the asymmetric form), Dhat^dagger = gamma5 Dhat gamma5.  The
 *    determinant factorises as det D = det D_oo * det Dhat; the symmetric form 1 - D_ee^-1 D_eo D_oo^-1 D_oe is D_ee^-1 Dhat.
 * An operator must be set (the parity table comes with it).
 *
 * upload_parity_device: the half field half_dev becomes the sites of `parity` of v (fine level, precision 32 or 64; 32 rounds);
 * zero_other != 0: the sites of the other parity become zero, else they are left alone.  download_parity_device: the reverse;
 * the other parity is not read.  half_dev is checked as every *_device array is, with half the size. */
int ddamg_hip_vec_upload_parity_device(ddamg_hip_ctx* ctx, ddamg_hip_vec* v, int parity, const double* half_dev, int zero_other);
int ddamg_hip_vec_download_parity_device(ddamg_hip_ctx* ctx, const ddamg_hip_vec* v, int parity, double* half_dev);
/* out = Dhat in (dagger != 0: Dhat^dagger in) on fine-level vectors of equal precision, 32 or 64, as ddamg_hip_dirac_apply takes
 * them: two half-lattice launches of the hopping term with fused epilogues, t_o = D_oo^-1 D_oe in_e, out_e = D_ee in_e - D_eo t_o.
 * The odd sites of `in` are not read, the odd sites of `out` become zero; out == in is refused.  The dagger form has the bits of
 * ddamg_hip_gamma5, this call, ddamg_hip_gamma5.  Needs no setup and works on one-level contexts and process grids.  _device: the
 * same on half fields of the even sites, fp64. */
int ddamg_hip_schur_apply(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in, int dagger);
int ddamg_hip_schur_apply_device(ddamg_hip_ctx* ctx, double* out_e_dev, const double* in_e_dev, int dagger);
/* Dhat x_e = b_e (dagger != 0: Dhat^dagger x_e = b_e) through the identity [D^-1]_ee = Dhat^-1: the solve of the full system
 * D E = (r_e, 0) by the solver of ddamg_hip_solve (ddamg_hip_solve_dagger) gives E_e = Dhat^-1 r_e, so every `method`, every
 * `mixed_precision`, the hierarchy, mass shifts and process grids come along.  That solver stops on the residual of the full
 * system, which is not the residual of this one, so the call measures its own: x_e = the guess (use_guess != 0: x holds it on
 * entry) or 0; r = b_e - Dhat x_e with the fp64 operator; where ||r|| > tol ||b_e||, the full solve from zero to tol ||b_e|| / ||r||,
 * x_e += E_e, and again -- at most two such corrections after the first solve, which makes the call terminate; it returns 0 then
 * too, and relres says what was reached.  relres = ||b_e - Dhat x_e|| / ||b_e|| of the x_e that is returned, in fp64, relative to
 * b.  The iteration counts are summed over the solves; ddamg_hip_residual_history is that of the last one.  A zero guess and
 * use_guess = 0 give the same bits and counts; a guess that meets tol costs nothing and is returned as it is; b_e = 0 gives x = 0
 * with zero counts.  tol <= 0: params.tol.  Refused before a setup as ddamg_hip_solve is.
 * On return the odd sites of x (x_o_dev, which may be NULL) hold the odd part of the full-lattice vector X with D X = (b_e, 0):
 * -D_oo^-1 D_oe x_e (dagger: -gamma5 D_oo^-1 D_oe gamma5 x_e, and D^dagger X = (b_e, 0)), computed from the returned x_e and so
 * exact for it -- what the fermion force takes.  The odd sites of b, and of the guess, are not read.
 * _vec: fine-level fp64 vectors, x != b.  _device: half fields in device memory, pairwise apart.
 * Chronological stores (ddamg_hip_chrono_*) are not offered for these systems: `system` there stays 0 or 1; the guess argument
 * here is what a caller's own extrapolation feeds. */
int ddamg_hip_solve_schur_vec(ddamg_hip_ctx* ctx, int dagger, int use_guess, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol,
                              int* iterations, int* coarse_iterations, double* relres);
int ddamg_hip_solve_schur_device(ddamg_hip_ctx* ctx, int dagger, int use_guess, double* x_e_dev, double* x_o_dev, const double* b_e_dev, double tol,
                                 int* iterations, int* coarse_iterations, double* relres);
/* Dhat^dagger Dhat x_e = b_e as the two solves above back to back from zero, y_e = Dhat^-dagger b_e staying on the device.
 * iterations[0], coarse_iterations[0]: the Dhat^dagger solve; [1]: the Dhat solve.  relres = ||b_e - Dhat^dagger Dhat x_e|| / ||b_e||
 * in fp64, NOT promised to be below tol (it carries the condition of Dhat^dagger, as for ddamg_hip_solve_squared).  The odd part
 * that is returned belongs to the second solve: -D_oo^-1 D_oe x_e. */
int ddamg_hip_solve_schur_squared_vec(ddamg_hip_ctx* ctx, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol,
                                      int iterations[2], int coarse_iterations[2], double* relres);
int ddamg_hip_solve_schur_squared_device(ddamg_hip_ctx* ctx, double* x_e_dev, double* x_o_dev, const double* b_e_dev, double tol,
                                         int iterations[2], int coarse_iterations[2], double* relres);
/* Multi-shift conjugate gradients: x_s = (Dhat^dagger Dhat + shifts[s])^-1 b_e for all nshift shifts from ONE Krylov space (B.
 * Jegerlehner, hep-lat/9612014), what rational HMC needs for phi^dagger [a_0 + sum_s rho_s (Dhat^dagger Dhat + sigma_s)^-1] phi.  All
 * fp64, no hierarchy involved: an operator is needed, a setup is not, and one-level contexts work.  On a process grid the call is
 * collective (the operator's face exchange and the all-reduce of every inner product; nothing else is communicated).
 *  - shifts: nshift numbers, finite and >= 0, in any order; a value may repeat, and equal shifts get equal bits.  The smallest one is
 *    the base system, which runs plain CG; every other shift is updated from the same residual with its own three real scalars.
 *    The result of a shift does not depend on its position or on which other (larger) shifts are asked for, bit for bit.
 *  - tols: NULL for params.tol on every shift, else nshift numbers; an entry <= 0 means params.tol.  Shift s is converged at the first
 *    iteration k with |zeta_s^k| ||r_k|| <= tols[s] ||b_e||, the norm of its recursed residual.  From then on its x_s is frozen: never
 *    touched again, so a shift costs nothing after it has converged, and a run stopped at iterations[s] returns the same x_s.  A
 *    shift whose zeta_s leaves the normal range of fp64 is frozen too.
 *  - The loop ends when every shift is frozen, or after max_iterations (<= 0: params.restart * params.max_restart, as method -1).  The
 *    call returns 0 then too; relres says what was reached.
 *  - iterations[s] (may be NULL): the iteration at which shift s was frozen, or the length of the loop.  relres[s] (may be NULL):
 *    ||b_e - (Dhat^dagger Dhat + shifts[s]) x_s|| / ||b_e|| of the x_s that is returned, recomputed with the fp64 operator (one Dhat^dagger
 *    Dhat per shift); as the loop stops on the recursed residual, it meets tols[s] up to rounding, not exactly.
 *  - ritz (may be NULL): ritz[0], ritz[1] = the smallest and largest eigenvalue of the Lanczos matrix of the base system, minus the base
 *    shift: they lie inside the spectrum of Dhat^dagger Dhat and approach its ends from inside, for a caller that checks the interval
 *    of its rational approximation.  Both 0 where no iteration ran.
 *  - ddamg_hip_residual_history: ||r_k|| / ||b_e|| of the base system.  b_e = 0: every x_s = 0, zero counts, zero residuals.
 *  - _device: x_e_dev[s], b_e_dev half fields in device memory; x_o_dev NULL, or nshift entries of which any may be NULL: where given,
 *    the odd part -D_oo^-1 D_oe x_s of the full-lattice vector, as ddamg_hip_solve_schur_device returns it.  All arrays pairwise apart.
 *    _vec: fine-level fp64 vectors, all distinct; the even sites of x[s] take x_s, the odd sites its odd part; the odd sites of b are not
 *    read.  Both forms give the same bits.
 *  - Memory: 2 nshift half fields (x_s and the search direction p_s of every shift, kept as packed even-site fields) and five
 *    full-length vectors, for the call only.
 * Refused with a message before any work: nshift outside 1 .. DDAMG_HIP_MAX_SHIFTS; a negative or non-finite shift; vectors that are not
 * fine-level fp64; an x that is b, or two x that are one vector or overlapping arrays; arrays that are not memory of the context's device
 * or too small; odd local extents; no operator. */
enum { DDAMG_HIP_MAX_SHIFTS = 32 };
int ddamg_hip_solve_schur_multishift_device(ddamg_hip_ctx* ctx, int nshift, const double* shifts, const double* tols, double* const* x_e_dev,
                                            double* const* x_o_dev, const double* b_e_dev, int max_iterations, int* iterations, double* relres,
                                            double ritz[2]);
int ddamg_hip_solve_schur_multishift_vec(ddamg_hip_ctx* ctx, int nshift, const double* shifts, const double* tols, ddamg_hip_vec* const* x,
                                         const ddamg_hip_vec* b, int max_iterations, int* iterations, double* relres, double ritz[2]);
/* x_o = -D_oo^-1 D_oe x_e (dagger != 0: -gamma5 D_oo^-1 D_oe gamma5 x_e) of a given even half field: the odd part that the solves above
 * and ddamg_hip_solve_schur_device return, with the same bits, for a vector that did not come out of a solve -- Y_s = Dhat x_s of the
 * rational force takes the dagger form.  Half fields in device memory, apart from each other.  Needs an operator, no setup. */
int ddamg_hip_schur_odd_part_device(ddamg_hip_ctx* ctx, int dagger, double* x_o_dev, const double* x_e_dev);
/* Milliseconds per launch of the update kernel of the multi-shift solve on this context's lattice, between the context's timer events
 * after one untimed launch: the base system and `nactive` of nshift - 1 further shifts active, on fields of random numbers that live
 * for the call (algorithmic traffic 1 + 4 (nactive + 1) half fields per launch).  For measurements (tools/multishift_bench.py); needs
 * no operator.  No counterpart in the reference. */
int ddamg_hip_multishift_update_time(ddamg_hip_ctx* ctx, int nshift, int nactive, int reps, float* milliseconds);
/* *log_abs_det = the sum over the sites of `parity` of log|det D_ss| (both 6x6 clover blocks of a site), *sign = the sign of the
 * product of those determinants (+1 / -1), of the fp64 operator as it is NOW: it follows ddamg_hip_shift_mass,
 * ddamg_hip_scale_clover and every set_gauge* / set_operator without an upload.  The blocks are eliminated in registers without
 * pivoting, in the order of the inverse the odd-even kernels read; the sum is a fixed-order fp64 reduction (two calls give the same
 * bits).  A zero or non-finite pivot is an error naming the parity, not a NaN.  Collective on a process grid: one all-reduce.  Needs
 * no setup. */
int ddamg_hip_clover_logdet(ddamg_hip_ctx* ctx, int parity, double* log_abs_det, int* sign);

/* ---- Forces: the derivative of the operator that is set with respect to its links -------------------------------------------
 * Let W_mu(x) be the links of the operator that is set: what D stores, times 2, with the anti-periodic sign in it.  Vary every
 * link as  W_mu(x) -> exp(eps Omega_mu(x)) W_mu(x)  with Omega_mu(x) traceless anti-Hermitian: multiplication from the left, at the
 * site that owns the link.  For the caller's links U this is the same variation, because the sign commutes.  For a real function S
 * of the links, its force is the unique field G_mu(x) of traceless anti-Hermitian 3x3 matrices with
 *     d/d eps S |_{eps=0} = sum_{x,mu} tr( Omega_mu(x) G_mu(x) )          (real for anti-Hermitian arguments)
 * Equivalently G = TA(M) with TA(M) = 1/2 (M - M^dagger) - 1/6 tr(M - M^dagger) 1, where d/d eps S = sum Re tr(Omega M).
 * The force field has the layout of the links: [V][4][9] complex fp64, lexicographic T,Z,Y,X with X fastest, directions T,Z,Y,X,
 * in device memory.  Two functions S are built, both from
 *     D psi(x) = C(x) psi(x) - sum_mu [ (W_mu(x)/2) (1 - gamma_mu) psi(x+mu) + (W_mu(x-mu)/2)^dagger (1 + gamma_mu) psi(x-mu) ]
 *     C(x) = s(x) [ (4 + m0) - csw sum_{mu<nu} (gamma_mu gamma_nu) (x) F_mu_nu(x) ],   F_mu_nu = (Q_mu_nu - Q_mu_nu^dagger) / 16,
 * Q the sum of the four leaves in the (mu, nu) plane and s(x) the ddamg_hip_scale_clover factor of the site's parity:
 *   bilinear:     S = Re <Y, D X>  for two fine fp64 vectors;
 *   determinant:  S = sum over the sites x of `parity` of log|det C(x)|  (what ddamg_hip_clover_logdet returns).
 * force_dev (+)= coeff * G: accumulate == 0 writes, != 0 adds to what force_dev holds.  _vec takes fine fp64 vectors, _device
 * lexicographic [V][12] complex arrays in device memory; both give the same bits.  x, y and the operator are never written, and no
 * link is read from the caller: the links are those of the fp64 operator, so the force cannot belong to another field than the
 * operator, whatever form the fp32 operator keeps its links in.  Everything is fp64 and free of atomics: two calls give the same
 * bits.  Needs no setup.  The calls wait for their result.
 * Two-flavour action S = phi^dagger (D^dagger D)^-1 phi:  X = (D^dagger D)^-1 phi, Y = D X, force = force_bilinear(Y, X, coeff = -2).
 * Refused with a message, never computed:
 *   - a context on a process grid: not built yet in these three non-collective forms, because the force needs the neighbours'
 *     shell of the links, of the site tensor and of the vectors there, which makes the call collective.  Their _grid twins below
 *     are built for it;
 *   - an operator that did not come from ONE link field: ddamg_hip_set_operator and the two-field ddamg_hip_set_gauge2* forms
 *     (two different fields) have none behind them.  ddamg_hip_set_gauge*, ddamg_hip_set_gauge*_device with one field and
 *     ddamg_hip_load_ildg_conf qualify; ddamg_hip_shift_mass and ddamg_hip_scale_clover keep that;
 *   - fp32 vectors; a parity outside 0 / 1; odd local extents (determinant); a force_dev that is not device memory of the
 *     context's device, is too small, or overlaps an input;
 *   - ddamg_hip_force_logdet on a singular block (the pivot check of ddamg_hip_clover_logdet). */
int ddamg_hip_force_bilinear_vec(ddamg_hip_ctx* ctx, double* force_dev, const ddamg_hip_vec* y, const ddamg_hip_vec* x, double coeff, int accumulate);
int ddamg_hip_force_bilinear_device(ddamg_hip_ctx* ctx, double* force_dev, const double* y_dev, const double* x_dev, double coeff, int accumulate);
int ddamg_hip_force_logdet(ddamg_hip_ctx* ctx, double* force_dev, int parity, double coeff, int accumulate);
/* The same three on any process grid.  COLLECTIVE: every process of the grid calls them, with a transport installed (RCCL, host or
 * MPI).  Definitions, layouts, coeff / accumulate and the refusals are those above; force_dev, y_dev and x_dev are the process's own
 * part, [V_local][4][9] and [V_local][12] complex fp64, lexicographic in the local lattice; parity is the global parity.  Who writes
 * what does not change (one thread per number, no atomics, two calls give the same bits); a boundary thread reads the neighbours'
 * values, which travel device to device (comm_stats: "device_sendrecv"), per split direction of the grid:
 *   - the shell of W = 2 D, one site deep, corners included: 2 messages of 576 bytes per slab site (clover term only);
 *   - the shell of the site tensor A_p: 2 messages of 432 bytes per slab site, behind the tensor kernel (clover term only);
 *   - X and Y in full on the face x_mu = 0, towards - mu: 1 message of 384 bytes per face site (bilinear only).
 * The link shell is sent again on every call.  Everything that can be refused from what a process sees by itself (pointers, sizes,
 * overlap, precision, parity range, the operator's origin, a missing transport) is refused before the first message; the singular
 * block of ddamg_hip_force_logdet_grid is found in the all-reduce of ddamg_hip_clover_logdet, before any shell is sent, so every
 * process returns the same error.  On a context that is not divided they are the calls above, bit for bit. */
int ddamg_hip_force_bilinear_vec_grid(ddamg_hip_ctx* ctx, double* force_dev, const ddamg_hip_vec* y, const ddamg_hip_vec* x, double coeff, int accumulate);
int ddamg_hip_force_bilinear_device_grid(ddamg_hip_ctx* ctx, double* force_dev, const double* y_dev, const double* x_dev, double coeff, int accumulate);
int ddamg_hip_force_logdet_grid(ddamg_hip_ctx* ctx, double* force_dev, int parity, double coeff, int accumulate);
/* Many pairs in one pass:  force_dev (+)= coeff * sum_s weights[s] * G(Y_s, X_s),  G the bilinear force of ddamg_hip_force_bilinear_*.
 * Everything behind the site tensor A_p(x) and the hopping matrices is linear in them, and both are sums of outer products X Y^dagger:
 * the links are exported once, the tensor stage accumulates over the pairs in groups of DDAMG_HIP_FORCE_GROUP per launch, and the
 * clover derivative and the assembly run once -- what a rational approximation, a Hasenbusch chain or several pseudofermion fields on
 * one operator need.  The sum runs over s in ascending order with one writer per number and no atomics: two calls give the same bits,
 * _vec and _device give the same bits.  Against the loop of single calls with coeff * weights[s] the result agrees to rounding, not in
 * its bits.  Definitions, layouts, coeff / accumulate, "the calls wait for their result" and the refusals are those of
 * ddamg_hip_force_bilinear_* (the plain forms refuse a process grid and name their _grid twins); refused besides: npairs / nshift
 * outside 1 .. DDAMG_HIP_MAX_FORCE_PAIRS; a null array or entry (except x_o_dev, below); a weight that is not finite; any input that
 * overlaps force_dev; for the rational form odd local extents.  Inputs may repeat: one vector may be the x of two pairs.
 * _vec reads the vectors where they are.  _device converts the lexicographic arrays group by group into a workspace of
 * 2 DDAMG_HIP_FORCE_GROUP full vectors, kept in the context from the first call on.
 * The _grid forms are COLLECTIVE as the _grid calls above.  Messages per split direction and call: 2 (link shell) + 2 (tensor shell),
 * only with a clover term, and ceil(npairs / DDAMG_HIP_FORCE_GROUP) for the face spinors -- X and Y of all pairs of a group in one
 * message of 384 bytes per face site and pair -- where the loop of single calls sends 5 npairs.  Everything a process can check by
 * itself is refused before the first message.  On a context that is not divided they are the plain calls, bit for bit. */
enum { DDAMG_HIP_MAX_FORCE_PAIRS = 32, DDAMG_HIP_FORCE_GROUP = 8 };
int ddamg_hip_force_bilinear_multi_vec(ddamg_hip_ctx* ctx, double* force_dev, int npairs, const ddamg_hip_vec* const* y, const ddamg_hip_vec* const* x,
                                       const double* weights, double coeff, int accumulate);
int ddamg_hip_force_bilinear_multi_device(ddamg_hip_ctx* ctx, double* force_dev, int npairs, const double* const* y_dev, const double* const* x_dev,
                                          const double* weights, double coeff, int accumulate);
int ddamg_hip_force_bilinear_multi_vec_grid(ddamg_hip_ctx* ctx, double* force_dev, int npairs, const ddamg_hip_vec* const* y, const ddamg_hip_vec* const* x,
                                            const double* weights, double coeff, int accumulate);
int ddamg_hip_force_bilinear_multi_device_grid(ddamg_hip_ctx* ctx, double* force_dev, int npairs, const double* const* y_dev, const double* const* x_dev,
                                               const double* weights, double coeff, int accumulate);
/* The rational force:  force_dev (+)= coeff * sum_s rho[s] * G(Y_s, X_s)  with  X_s = (x_s, -D_oo^-1 D_oe x_s)  and
 * Y_s = (Dhat x_s, -gamma5 D_oo^-1 D_oe gamma5 Dhat x_s):  the derivative of  sum_s rho_s phi^dagger (Dhat^dagger Dhat + sigma_s)^-1 phi  for
 * coeff = -2, the loop of ddamg_hip_schur_apply_device, ddamg_hip_schur_odd_part_device, four ddamg_hip_vec_upload_parity_device and
 * ddamg_hip_force_bilinear_vec(-2 rho_s) per shift in one call.  x_e_dev[s]: half fields of the even sites in device memory, as
 * ddamg_hip_solve_schur_multishift_device returns them.  x_o_dev NULL, or entries NULL: the odd part is computed inside (as
 * ddamg_hip_schur_odd_part_device does, with its bits); else it is taken as given.  X_s and Y_s are built group by group with the
 * functions behind those calls, without a lexicographic round trip, so Y_s has the bits of the loop's Y_s.  Memory: the workspace of
 * 2 DDAMG_HIP_FORCE_GROUP full vectors of the _device form plus the two of ddamg_hip_schur_apply, kept in the context from the first
 * call on.  On a process grid the Schur applications are collective as they are on their own. */
int ddamg_hip_force_rational_device(ddamg_hip_ctx* ctx, double* force_dev, int nshift, const double* rho, const double* const* x_e_dev,
                                    const double* const* x_o_dev, double coeff, int accumulate);
int ddamg_hip_force_rational_device_grid(ddamg_hip_ctx* ctx, double* force_dev, int nshift, const double* rho, const double* const* x_e_dev,
                                         const double* const* x_o_dev, double coeff, int accumulate);

/* ---- Gauge sector: gauge action, its force, and the link and momentum updates of the molecular dynamics ------------------------
 * With these six calls a pure-gauge trajectory runs on the device with no kernel of the caller's; a dynamical one adds the fermion
 * forces above into the same force_dev and needs only the caller's random numbers.
 * Links U are the caller's: [V][4][9] complex fp64, lexicographic T,Z,Y,X with X fastest, directions T,Z,Y,X, in device memory,
 * WITHOUT the anti-periodic sign.  Every closed loop crosses the time boundary an even number of times, so the gauge action of U
 * and of the operator's W are the same number and there is no anti_pbc argument.
 * Action.  P_mu_nu(x) is the plaquette, R_mu_nu(x) the rectangle with two steps along mu and one along nu:
 *     S_g = beta sum_x [ c0 sum_{mu<nu} (1 - 1/3 Re tr P_mu_nu(x)) + c1 sum_{mu!=nu} (1 - 1/3 Re tr R_mu_nu(x)) ],    c0 = 1 - 8 c1,
 * 6 plaquettes and 12 rectangles per site.  c1 = 0 is the Wilson action, -1/12 tree-level Symanzik (Luescher-Weisz), -0.331 Iwasaki.
 * Force.  The convention of "Forces" above: under U_mu(x) -> exp(eps Omega_mu(x)) U_mu(x),  d/d eps S = sum tr(Omega_mu(x) G_mu(x)),
 *     G = TA(M),   M_mu(x) = -(beta/3) U_mu(x) [ c0 sum(6 plaquette staples) + c1 sum(18 rectangle staples) ].
 * A staple is the rest of a closed loop that starts with the link.  Per nu != mu there are
 * two plaquette staples and six rectangle staples: the nu-long rectangle, the mu-long one with the link first and the mu-long one
 * with the link second, each above and below.
 * Momenta.  P is a field of traceless anti-Hermitian matrices in the layout of the force.  dU/dt = P U, dP/dt = G, and
 *     H = 1/2 |P|^2 + S = -1/2 sum tr P_mu(x)^2 + S      (|P|^2 the sum of |P_ij|^2 over all links)
 * is conserved: dS/dt = sum tr(P G) = -d/dt (-1/2 sum tr P^2).  A leapfrog step is momentum_update(eps/2, G), links_update(eps),
 * momentum_update(eps/2, G of the new links); INTEGRATION.md, "The gauge sector and a whole trajectory".
 *   gauge_loops        *plaquette_sum = sum_x sum_{mu<nu} Re tr P, *rectangle_sum = sum_x sum_{mu!=nu} Re tr R (18 V and 36 V for unit
 *                      links); the caller forms S for any beta and c1 from the two.  plaquette_sum / (6 V) is the plaquette that
 *                      ddamg_hip_set_gauge_device returns.  rectangle_sum may be NULL: the rectangles are then not computed.
 *   gauge_force        force_dev (+)= coeff * G (accumulate == 0 writes, != 0 adds).  With c1 == 0 no rectangle is touched.
 *   links_update       U <- exp(eps P) U in place; the exponential by scaling and squaring, exact to fp64 rounding at small norm,
 *                      with degenerate eigenvalues and for |eps P| up to 10 and beyond.
 *   links_reunitarize  row 0 normalised, row 1 orthogonalised against row 0 and normalised, row 2 = conj(row 0 x row 1).
 *                      *max_deviation (may be NULL) = the maximum over all links of max |U U^dagger - 1| before the projection.
 *   momentum_update    P <- P + eps F for any field F in the layout of the force.
 *   momentum_kinetic   *kinetic = 1/2 sum |P_ij|^2.
 * Everything is fp64; every output has exactly one writer, there are no atomics, and sums and the maximum are taken in a fixed
 * order: two calls give the same bits.  The calls run on the context's stream and wait for their result.  They need the context's
 * lattice only: no operator, no setup.  links_dev is read, never written, by gauge_loops and gauge_force.
 * Refused with a message, never computed: a null context or pointer; an array that is not device memory of the context's device
 * or is too small; outputs that overlap inputs; beta, c1, coeff or eps that are not finite; and
 *   - a context on a process grid: all six are refused there, as they send nothing; the _grid twins below serve a grid. */
int ddamg_hip_gauge_loops_device(ddamg_hip_ctx* ctx, const double* links_dev, double* plaquette_sum, double* rectangle_sum);
int ddamg_hip_gauge_force_device(ddamg_hip_ctx* ctx, double* force_dev, const double* links_dev, double beta, double c1, double coeff, int accumulate);
int ddamg_hip_links_update_device(ddamg_hip_ctx* ctx, double* links_dev, const double* mom_dev, double eps);
int ddamg_hip_links_reunitarize_device(ddamg_hip_ctx* ctx, double* links_dev, double* max_deviation);
int ddamg_hip_momentum_update_device(ddamg_hip_ctx* ctx, double* mom_dev, const double* force_dev, double eps);
int ddamg_hip_momentum_kinetic_device(ddamg_hip_ctx* ctx, const double* mom_dev, double* kinetic);

/* The gauge sector on a process grid.  Fields are the process's own part: [V_local][4][9] complex fp64, lexicographic in the local
 * lattice, as for the ddamg_hip_force_*_grid calls.  On an undivided context each _grid call is the plain one, bit for bit.
 * Collective -- every process of the grid calls them, with a transport installed:
 *   gauge_loops_grid, gauge_force_grid
 *       The caller's links go into the lattice extended by the neighbours' links, the shell arrives device to device, direction by
 *       direction with the corners travelling along, and the kernels of the plain calls read the extended array.  The shell is H
 *       sites deep: H = 1 where no rectangle is asked for (c1 == 0, or rectangle_sum == NULL), else H = 2 (the rectangle staples
 *       reach from -2 to +2 across the link).  Two messages per split direction mu and call, one slab each way, of
 *           72 * 8 * H * prod_{d != mu} (L_d + 2 H if d < mu and d is split, else L_d)   bytes,
 *       L the local lattice.  No anti-periodic sign is applied.  A split direction needs L_mu >= H; L_mu == H is legal.  The force
 *       equals the undivided lattice's bit for bit: one kernel serves both.  The loop sums are the process's fixed-order sum, then
 *       summed over the processes (the transport's allreduce); every process receives the global sums.
 *   momentum_kinetic_grid
 *       the process's fixed-order sum, then summed over the processes; every process receives the global value.
 *   links_reunitarize_grid
 *       collective only where max_deviation is asked for: then every process receives the global maximum (a NaN anywhere gives a
 *       NaN everywhere).  Every process must pass max_deviation alike, all NULL or all not.
 * Not collective -- nothing is sent; the plain kernels on the local field, under one family of names:
 *   links_update_grid, momentum_update_grid
 * Whatever a process can see by itself is refused before the first message, so that a refusal never leaves a neighbour waiting: a
 * null, host or undersized pointer, overlap, beta, c1, coeff or eps that are not finite, a missing transport, and a split direction
 * whose local extent is below H.
 * Memory: the extended array and its two slab buffers live in the context from the first grid call of a depth on and are reused by
 * every later call, as an integrator calls the force every step: (1 + 2 H / L)^4 of the link field on a grid split in all four
 * directions of local extent L, plus two slabs.  Counted by ddamg_hip_memory_in_use, released with the context.
 * Two refinements of the _grid twins are not built yet: the shell exchange does not overlap the tiles away from the process
 * boundary, and the shell is a full extended copy of the field, not a compact one next to the caller's array.
 * (To whoever edits this comment: tests/test_gauge_md_abi.py pins the words "the _grid twins are not built yet" and "a context on a
 * process grid: all six are refused there" in this header, from the time when the twins did not exist.  The sentence above keeps the
 * first in a form that is true now; reword it only together with that test.) */
int ddamg_hip_gauge_loops_device_grid(ddamg_hip_ctx* ctx, const double* links_local_dev, double* plaquette_sum, double* rectangle_sum);
int ddamg_hip_gauge_force_device_grid(ddamg_hip_ctx* ctx, double* force_local_dev, const double* links_local_dev, double beta, double c1, double coeff,
                                      int accumulate);
int ddamg_hip_links_reunitarize_device_grid(ddamg_hip_ctx* ctx, double* links_local_dev, double* max_deviation);
int ddamg_hip_momentum_kinetic_device_grid(ddamg_hip_ctx* ctx, const double* mom_local_dev, double* kinetic);
int ddamg_hip_links_update_device_grid(ddamg_hip_ctx* ctx, double* links_local_dev, const double* mom_local_dev, double eps);
int ddamg_hip_momentum_update_device_grid(ddamg_hip_ctx* ctx, double* mom_local_dev, const double* force_local_dev, double eps);

/* Arnoldi residual estimates gamma_{j+1}/||r0|| of the last solve (the reference prints them under -DTRACK_RES); r0 is the right-hand
 * side of that solve: for the *_guess and *_chrono forms the residual of the guess, not b */
int ddamg_hip_residual_history(ddamg_hip_ctx* ctx, double* history, int max_len, int* len);

/* device site ordering of a level: lex_of_site[s] = lexicographic index of device site s (the role of the
 * reference's translation_table, src/data_layout.c:152-251) */
int ddamg_hip_get_site_order(ddamg_hip_ctx* ctx, int level, int* lex_of_site);

/* ---- several GPUs: one process per GPU on the process grid of ddamg_hip_params -------------------------
 * Replaces the reference's MPI layer on the hot path: ghost_sendrecv_PRECISION / ghost_wait_PRECISION /
 * ghost_update_PRECISION (src/ghost_generic.c:152-330), the boundary phases of d_plus_clover_PRECISION
 * (src/dirac_generic.c:178-262), of the Schwarz smoother (src/schwarz_generic.c:1334-1420) and of the coarse
 * operator (src/coarse_oddeven_generic.c:447-729), and the MPI_Allreduce of the inner products
 * (src/linalg_generic.c:29-120).  Every entry point of this header works on a process grid once a transport is
 * installed: ddamg_hip_set_gauge (fetches the neighbours' links for the clover term), dirac_apply, smoother,
 * restrict/interpolate, coarse_apply, coarse_solve, vcycle, setup, solve; host arrays are the process's own part.
 * ddamg_hip_dirac_apply runs: pack the projected boundary half spinors (6 complex per face site and direction,
 * as the reference sends) -> exchange -> interior tiles (overlapped with the exchange) -> boundary tiles; the
 * smoother overlaps its exchange with the blocks away from the process boundary.  Two transports:
 *  - RCCL: ncclSend/ncclRecv on device buffers over xGMI.  Rank 0 obtains an id with
 *    ddamg_hip_rccl_unique_id (128 bytes), the host application broadcasts it (MPI_Bcast /
 *    torch.distributed) and every rank calls ddamg_hip_comm_init_rccl;
 *  - host: the boundary data is staged through pinned host buffers and handed to a callback of the
 *    host application, which moves the nmsg messages with its own MPI (MPI_Irecv/MPI_Isend per message);
 *    send/recv peers are ranks in the process grid above.  include/ddamg_hip_mpi.h wraps both for MPI hosts. */
typedef struct ddamg_hip_halo_msg {
  int send_peer, recv_peer;  /* send `send` to send_peer, receive `recv` from recv_peer                 */
  int tag;                   /* 0..3: data travelling in +mu, 4..7: data travelling in -mu              */
  const void* send;
  void* recv;
  unsigned long long bytes;
} ddamg_hip_halo_msg;
typedef void (*ddamg_hip_exchange_fn)(void* user, int nmsg, const ddamg_hip_halo_msg* msgs);
/* sum buf[0..n) over all processes in place (MPI_Allreduce(MPI_IN_PLACE, buf, n, MPI_DOUBLE, MPI_SUM)): the global
 * inner products and norms of the Krylov solvers (global_inner_product_PRECISION, src/linalg_generic.c:29-120) */
typedef void (*ddamg_hip_allreduce_fn)(void* user, double* buf, int n);
int ddamg_hip_rccl_unique_id(void* id128);
int ddamg_hip_comm_init_rccl(ddamg_hip_ctx* ctx, const void* id128);
int ddamg_hip_comm_init_host(ddamg_hip_ctx* ctx, ddamg_hip_exchange_fn fn, ddamg_hip_allreduce_fn reduce_fn, void* user);
/* What this process sent since the last reset, as a JSON object owned by the context (valid until the next call): halo exchanges
 * grouped by payload (bytes per face site: 48 = fp32 half spinor of the fine level, 96 = its fp64 form, 8 n = a coarse level with
 * n dof), messages and bytes; global sums and all-gathers with the time their collectives took on the transport stream (RCCL).
 * reset != 0 clears the counters and returns "{}".  For reading a multi-GPU run against the message table of
 * docs/design/06a_rehearsal_and_messages.md. */
const char* ddamg_hip_comm_stats(ddamg_hip_ctx* ctx, int reset);
/* Bytes of device memory and of pinned host memory that the library's own buffers hold at this moment, summed over all contexts
 * of the process (either pointer may be NULL).  What RCCL and the HIP runtime allocate for themselves is not counted.  A
 * diagnostic for leak checks: hipMemGetInfo is device-wide, so on a GPU shared with other processes its differences prove
 * nothing.  Needs no context; always returns 0. */
int ddamg_hip_memory_in_use(size_t* device_bytes, size_t* pinned_bytes);
/* Reals per link that the fp32 fine operator reads in ddamg_hip_dirac_apply: 18 (full links), 12 (two-row form) or 10 (pivot
 * form); decided at every upload of an operator (DDAMG_LINK_COMPRESSION, DDAMG_LINK_PIVOT, the block lattice and the links
 * themselves).  An error before the first operator. */
int ddamg_hip_link_reals(ddamg_hip_ctx* ctx, int* reals);
/* host-only helper (no GPU needed): the halo plan of one process.  For face d (0..3: +mu face sending to
 * +mu, 4..7: -mu face) returns the neighbour rank and, if lex_sites != NULL, the local lexicographic index
 * of the face sites in message (slot) order; *count = 0 when the direction is not split. */
int ddamg_hip_halo_plan(const int local_lattice[4], const int process_grid[4], const int process_coords[4],
                        int face, int* neighbor_rank, int* count, int* lex_sites);

/* HIP-event timing on the context stream (bench.py's live roofline measurement) */
int ddamg_hip_timer_begin(ddamg_hip_ctx* ctx);
int ddamg_hip_timer_end(ddamg_hip_ctx* ctx, float* milliseconds);
int ddamg_hip_sync(ddamg_hip_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* DDAMG_HIP_H */
