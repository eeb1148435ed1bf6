/* ddamg_hip_io.h -- the reference's on-disk formats for gauge configurations and spinor / test-vector files, read and
 * written directly by every process for its own part of the lattice (host code only: no GPU, no MPI).
 *
 * Replaces, for the data either side of the hot path:
 *   read_conf                       src/io.c:459-563   one file, rank 0 reads and scatters rows of X
 *   vector_io (_READ / _WRITE)      src/io.c:704-846   one spinor, optional text header, lexicographic sites
 *   vector_io_single_file           src/io.c:951-1124  n spinors behind one header (test vectors: setup persistence)
 *   write_header                    src/io.c:671-702
 *   read_conf_multi                 src/io.c:566-668   one file per process of the grid, <base>.pt<T>pz<Z>py<Y>px<X>
 * and, for the reference's `format: 1` build (-DHAVE_LIME, src/lime_io.c, chosen in src/main.c:69-81), without the c-lime library:
 *   lime_read_conf                  src/lime_io.c:222-337  ILDG configuration in a LIME container, fp64 or fp32
 *   lime_read_vector / _write_vector  src/lime_io.c:339-535  one spinor as SciDAC/ETMC records
 *   lime_read_info / _check_info / _write_info  src/lime_io.c:94-217
 * Not covered: the HDF5 build.
 *
 * Layouts (all little endian unless `big_endian` is set, the reference's -DBIG_ENDIAN_CNFG / -DBIG_ENDIAN_TV builds):
 *   configuration: int32 T,Z,Y,X ; double plaquette ; then for t,z,y,x (x fastest): 4 directions (T,Z,Y,X) x 3x3 complex
 *                  doubles, row major = 72 doubles per site.  The anti-periodic sign of the last time slice is NOT applied
 *                  here (ddamg_hip_set_gauge takes it as an argument).
 *   vectors:       optional "<header>\n ... </header>\n" text block, then per vector, for t,z,y,x: 12 complex doubles.
 * A process with coordinates `process_coords` on the grid `process_grid` (T,Z,Y,X; rank order as in ddamg_hip.h) owns the
 * sub-lattice global/process_grid at that position; its part is returned / taken in local lexicographic order. */
#ifndef DDAMG_HIP_IO_H
#define DDAMG_HIP_IO_H
#ifdef __cplusplus
extern "C" {
#endif

/* text of the last failure of a call below (static buffer, per thread) */
const char* ddamg_hip_io_last_error(void);

/* lattice extents and plaquette stored in a configuration file.  Returns 0, or -1 on failure. */
int ddamg_hip_conf_info(const char* path, int big_endian, int lattice_out[4], double* plaq_out);

/* gauge_local: [V_local][4][9][2] doubles.  The file's extents must equal global_lattice (ASSERT in src/io.c:497-498). */
int ddamg_hip_read_conf(const char* path, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                        int big_endian, double* gauge_local, double* plaq_out);
/* the same layout written out (single file; every process writes its own rows, the process at the origin the header) */
int ddamg_hip_write_conf(const char* path, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                         int big_endian, const double* gauge_local, double plaq);

/* read_conf_multi (src/io.c:566-668): the part of the process at process_coords from the file <base>.pt<T>pz<Z>py<Y>px<X>, which
 * carries the header of the global lattice and that process's links in local lexicographic order; the writer is its inverse
 * (every process writes its own file). */
int ddamg_hip_read_conf_multi(const char* base, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                              int big_endian, double* gauge_local, double* plaq_out);
int ddamg_hip_write_conf_multi(const char* base, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                               int big_endian, const double* gauge_local, double plaq);

/* fields of write_header; strings may be NULL (written as empty) */
typedef struct ddamg_hip_vector_header {
  const char* vector_type;        /* second line of the header: "test vectors", or the file name for single spinors */
  double m0, csw, clov_plaq, hopp_plaq;
  const char* clov_conf_name;
  const char* hopp_conf_name;
  int has_eigenvalues;            /* write the "eigenvalues:" line from `eigenvalues` (2 n doubles) */
  const double* eigenvalues;
} ddamg_hip_vector_header;

/* vectors_local: [n][V_local][12][2] doubles.  A file without header is accepted when n == 1 (src/io.c:735-743). */
int ddamg_hip_read_vectors(const char* path, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                           int n, int big_endian, double* vectors_local);
/* header == NULL writes the bare data (readable as a single spinor only) */
int ddamg_hip_write_vectors(const char* path, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                            int n, int big_endian, const ddamg_hip_vector_header* header, const double* vectors_local);

/* ---- ILDG configurations and SciDAC/ETMC spinors in the LIME container ---------------------------------------------------
 * A LIME file is a sequence of records: a 144-byte header (magic 45 67 89 ab; big-endian 16-bit version 1; one byte of flags,
 * 0x80 message begin, 0x40 message end; one reserved byte; big-endian 64-bit data length; the record type as NUL-filled ASCII in
 * 128 bytes), the data, zeros up to a multiple of 8 bytes.  Written here with every record a message of its own (flags 0xC0), as
 * the reference writes them (limeCreateHeader(1, 1, ...), src/lime_io.c:174-208).
 *   configuration: record "ildg-format" (XML; <precision> 32 or 64, <lx> <ly> <lz> <lt>, found by searching for the tags as the
 *                  reference does, src/lime_io.c:110-121), optional record "xlf-info" (text with "plaquette = <number>", the
 *                  average plaquette in [0,1], src/lime_io.c:137-143), record "ildg-binary-data": for t,z,y,x (x fastest) the four
 *                  links of the site in the order X,Y,Z,T -- the reverse of this library's T,Z,Y,X (src/lime_io.c:35-48) -- each
 *                  3x3 row-major complex, big-endian IEEE.  No anti-periodic sign in the file.
 *   vector:        records "vector-type", "etmc-propagator-format" (or "etmc-source-format": XML with precision, flavours,
 *                  lx..lt, spin, colour), "dd_alpha_amg-header", "scidac-binary-data": [t][z][y][x][12] complex, big-endian, in
 *                  this library's spin-colour order (the reference does not permute it, src/lime_io.c:395-428). */
struct ddamg_hip_lime_info {
  int kind;               /* 0: no binary record known here, 1: configuration ("ildg-binary-data"), 2: vector ("scidac-binary-data") */
  int precision;          /* 32 or 64 from the format record that belongs to `kind`; 0 if there is none */
  int lattice[4];         /* T,Z,Y,X from the same record; 0 where a tag is missing */
  int has_plaquette;      /* an "xlf-info" record with "plaquette =" was found */
  double plaquette;       /* the file's number, the average plaquette in [0,1] */
  long long data_offset;  /* first byte of the binary record's data */
  long long data_length;  /* its length in bytes as the record header states it */
  int num_records;
};
/* scans all record headers of the file.  Returns 0, or -1 on failure (cannot open, not a LIME file, file ends early). */
int ddamg_hip_lime_info(const char* path, struct ddamg_hip_lime_info* out);

/* gauge_local: [V_local][4][9][2] doubles in this library's direction order, from an fp64 or fp32 file (fp32 widened exactly).
 * *plaq_out (may be NULL) is three times the file's number, in [0,3] as ddamg_hip_set_gauge returns it; *has_plaq_out (may be
 * NULL) tells whether the file has one.  The record length must be volume x 72 x the precision's bytes (lime_check_info,
 * src/lime_io.c:152-161).  Nothing is written to gauge_local when the call fails before the first row is read. */
int ddamg_hip_read_ildg_conf(const char* path, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                             double* gauge_local, double* plaq_out, int* has_plaq_out);
/* records "ildg-format", "xlf-info" (plaquette = plaq / 3 with 17 significant digits), "ildg-binary-data"; precision 64, or 32
 * (links rounded to nearest).  Every process writes its own rows, the process at the origin the record headers and texts. */
int ddamg_hip_write_ildg_conf(const char* path, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                              int precision, const double* gauge_local, double plaq);

/* vector_local: [V_local][12][2] doubles.  Accepts fp64 and fp32 files and both ETMC record names; refuses anything but flavours 1,
 * spin 4, colour 3. */
int ddamg_hip_read_lime_vector(const char* path, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                               double* vector_local);
/* the reference's four records (lime_write_info, src/lime_io.c:163-217), fp64.  The "dd_alpha_amg-header" text carries the fields
 * of `header` (NULL: all empty / zero) and the global and local extents; the offset of the data follows from the text, so every
 * process passes the same header (and, to ddamg_hip_write_ildg_conf, the same plaquette). */
int ddamg_hip_write_lime_vector(const char* path, const int global_lattice[4], const int process_grid[4], const int process_coords[4],
                                const ddamg_hip_vector_header* header, const double* vector_local);

#ifdef __cplusplus
}
#endif
#endif
