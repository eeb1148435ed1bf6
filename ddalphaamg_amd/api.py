"""ctypes mirror of include/ddamg_hip.h (same names, argument meaning and error behaviour)."""
import ctypes, os, re
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DDAMG_HIP_LIBRARY: another build of the same library (A/B measurements of a kernel change on one GPU box); never a fallback
_LIBNAME = os.environ.get("DDAMG_HIP_LIBRARY") or os.path.join(_HERE, "libddamg_hip.so")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddamg_hip.h")
MAX_LEVELS = 4
MAX_FORCE_PAIRS = 32      # DDAMG_HIP_MAX_FORCE_PAIRS
FORCE_GROUP = 8           # DDAMG_HIP_FORCE_GROUP: the pairs of one launch of the many-pair force


class DDAMGError(RuntimeError):
    pass


class Params(ctypes.Structure):
    """struct ddamg_hip_params (include/ddamg_hip.h); lattices in T,Z,Y,X order."""
    _fields_ = [
        ("num_levels", ctypes.c_int),
        ("local_lattice", (ctypes.c_int * 4) * MAX_LEVELS),
        ("block_lattice", (ctypes.c_int * 4) * MAX_LEVELS),
        ("num_vect", ctypes.c_int * MAX_LEVELS),
        ("post_smooth_iter", ctypes.c_int * MAX_LEVELS),
        ("block_iter", ctypes.c_int * MAX_LEVELS),
        ("setup_iter", ctypes.c_int * MAX_LEVELS),
        ("restart", ctypes.c_int), ("max_restart", ctypes.c_int),
        ("tol", ctypes.c_double),
        ("coarse_iter", ctypes.c_int), ("coarse_restart", ctypes.c_int),
        ("coarse_tol", ctypes.c_double),
        ("kcycle", ctypes.c_int), ("kcycle_restart", ctypes.c_int), ("kcycle_max_restart", ctypes.c_int),
        ("kcycle_tol", ctypes.c_double),
        ("mixed_precision", ctypes.c_int),
        ("odd_even", ctypes.c_int),
        ("method", ctypes.c_int),
        ("m0", ctypes.c_double), ("csw", ctypes.c_double),
        ("device", ctypes.c_int),
        ("process_grid", ctypes.c_int * 4),
        ("process_coords", ctypes.c_int * 4),
        ("test_vector_rng", ctypes.c_int),
        ("rng_seed", ctypes.c_ulonglong),
        ("gather_coarsest", ctypes.c_int),
    ]


class HaloMsg(ctypes.Structure):
    """struct ddamg_hip_halo_msg"""
    _fields_ = [
        ("send_peer", ctypes.c_int), ("recv_peer", ctypes.c_int), ("tag", ctypes.c_int),
        ("send", ctypes.c_void_p), ("recv", ctypes.c_void_p), ("bytes", ctypes.c_ulonglong),
    ]


EXCHANGE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(HaloMsg))
ALLREDUCE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int)


_lib = None


def library_path():
    return _LIBNAME


def declared_symbols():
    """every function include/ddamg_hip.h and include/ddamg_hip_io.h declare"""
    txt = open(_HEADER).read() + open(os.path.join(os.path.dirname(_HEADER), "ddamg_hip_io.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ddamg_hip_[a-z0-9_]+)\s*\(", txt)))


def load_library():
    """Load libddamg_hip.so; raises DDAMGError (never falls back to anything) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIBNAME):
        raise DDAMGError(f"{_LIBNAME} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                         "there is no CPU fallback for the HIP path")
    lib = ctypes.CDLL(_LIBNAME)
    vp = ctypes.c_void_p
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int)
    lib.ddamg_hip_last_error.restype = ctypes.c_char_p
    lib.ddamg_hip_comm_stats.restype = ctypes.c_char_p
    lib.ddamg_hip_comm_stats.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ddamg_hip_default_params.argtypes = [ctypes.POINTER(Params)]
    lib.ddamg_hip_default_params.restype = None
    sigs = {
        "ddamg_hip_create": [ctypes.POINTER(Params), ctypes.POINTER(vp)],
        "ddamg_hip_destroy": [vp],
        "ddamg_hip_set_gauge": [vp, dp, ctypes.c_int, dp],
        "ddamg_hip_set_gauge2": [vp, dp, dp, ctypes.c_int, dp],
        "ddamg_hip_set_gauge_device": [vp, dp, ctypes.c_int, dp],
        "ddamg_hip_set_gauge2_device": [vp, dp, dp, ctypes.c_int, dp],
        "ddamg_hip_set_gauge_device_grid": [vp, dp, ctypes.c_int, dp],
        "ddamg_hip_set_gauge2_device_grid": [vp, dp, dp, ctypes.c_int, dp],
        "ddamg_hip_ildg_to_links_device": [vp, vp, ctypes.c_int, ctypes.c_longlong, dp],
        "ddamg_hip_links_to_ildg_device": [vp, dp, ctypes.c_int, ctypes.c_longlong, vp],
        "ddamg_hip_load_ildg_conf": [vp, ctypes.c_char_p, ctypes.c_int, dp, dp, ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_clover_kernel_time": [vp, dp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), dp],
        "ddamg_hip_vec_upload_device": [vp, vp, dp],
        "ddamg_hip_vec_download_device": [vp, vp, dp],
        "ddamg_hip_solve_device": [vp, dp, dp, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), dp],
        "ddamg_hip_preconditioner_device": [vp, dp, dp],
        "ddamg_hip_set_operator": [vp, dp, dp],
        "ddamg_hip_shift_mass": [vp, ctypes.c_double],
        "ddamg_hip_setup_at_mass": [vp, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_scale_clover": [vp, ctypes.c_double, ctypes.c_double],
        "ddamg_hip_get_operator": [vp, dp, dp],
        "ddamg_hip_vec_create": [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)],
        "ddamg_hip_vec_destroy": [vp, vp],
        "ddamg_hip_vec_upload": [vp, vp, dp],
        "ddamg_hip_vec_download": [vp, vp, dp],
        "ddamg_hip_dirac_apply": [vp, vp, vp],
        "ddamg_hip_dirac_apply_dagger": [vp, vp, vp],
        "ddamg_hip_gamma5": [vp, vp, vp],
        "ddamg_hip_vec_copy": [vp, vp, vp],
        "ddamg_hip_vec_axpy": [vp, vp, vp, vp, ctypes.c_double, ctypes.c_double],
        "ddamg_hip_vec_dot": [vp, vp, vp, dp, dp, dp],
        "ddamg_hip_setup": [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_setup_update": [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_set_test_vectors": [vp, dp, ctypes.c_int],
        "ddamg_hip_get_interpolation": [vp, dp],
        "ddamg_hip_get_test_vectors": [vp, dp],
        "ddamg_hip_get_coarse_operator": [vp, dp, dp],
        "ddamg_hip_set_coarse_operator": [vp, dp, dp],
        "ddamg_hip_get_coarse_operator_level": [vp, ctypes.c_int, dp, dp],
        "ddamg_hip_set_coarse_operator_level": [vp, ctypes.c_int, dp, dp],
        "ddamg_hip_set_interpolation_level": [vp, ctypes.c_int, dp],
        "ddamg_hip_kcycle": [vp, vp, vp, ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_coarse_apply_many": [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp)],
        "ddamg_hip_smoother_many": [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int],
        "ddamg_hip_vcycle_many": [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp)],
        "ddamg_hip_kcycle_many": [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_smoother": [vp, vp, vp, ctypes.c_int, ctypes.c_int],
        "ddamg_hip_restrict": [vp, vp, vp],
        "ddamg_hip_interpolate": [vp, vp, vp, ctypes.c_int],
        "ddamg_hip_coarse_apply": [vp, vp, vp],
        "ddamg_hip_coarse_solve": [vp, vp, vp, ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_set_coarse_storage": [vp, ctypes.c_int],
        "ddamg_hip_set_transfer_storage": [vp, ctypes.c_int],
        "ddamg_hip_set_intermediate_storage": [vp, ctypes.c_int],
        "ddamg_hip_coarse_hop": [vp, vp, vp, ctypes.c_int, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_coarse_self_mul": [vp, vp, vp, ctypes.c_int, ctypes.c_int],
        "ddamg_hip_coarse_solve_many": [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_vcycle": [vp, vp, vp],
        "ddamg_hip_solve": [vp, dp, dp, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), dp],
        "ddamg_hip_solve_vec": [vp, vp, vp, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), dp],
        "ddamg_hip_solve_dagger": [vp, dp, dp, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), dp],
        "ddamg_hip_solve_dagger_vec": [vp, vp, vp, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), dp],
        "ddamg_hip_solve_dagger_device": [vp, dp, dp, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), dp],
        "ddamg_hip_solve_squared": [vp, dp, dp, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), dp],
        "ddamg_hip_solve_squared_vec": [vp, vp, vp, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), dp],
        "ddamg_hip_solve_squared_device": [vp, dp, dp, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), dp],
        "ddamg_hip_solve_guess": [vp, ctypes.c_int, dp, dp, ctypes.c_double, ip, ip, dp, dp],
        "ddamg_hip_solve_guess_vec": [vp, ctypes.c_int, vp, vp, ctypes.c_double, ip, ip, dp, dp],
        "ddamg_hip_solve_guess_device": [vp, ctypes.c_int, dp, dp, ctypes.c_double, ip, ip, dp, dp],
        "ddamg_hip_chrono_create": [vp, ctypes.c_int, ctypes.POINTER(vp)],
        "ddamg_hip_chrono_destroy": [vp, vp],
        "ddamg_hip_chrono_reset": [vp, vp],
        "ddamg_hip_chrono_count": [vp, vp, ip],
        "ddamg_hip_chrono_push_vec": [vp, vp, vp],
        "ddamg_hip_chrono_guess_vec": [vp, vp, ctypes.c_int, vp, vp, ip, dp],
        "ddamg_hip_solve_chrono_vec": [vp, vp, ctypes.c_int, vp, vp, ctypes.c_double, ip, ip, dp, dp],
        "ddamg_hip_solve_chrono_device": [vp, vp, ctypes.c_int, dp, dp, ctypes.c_double, ip, ip, dp, dp],
        "ddamg_hip_solve_squared_chrono_vec": [vp, vp, vp, vp, vp, ctypes.c_double, ip, ip, dp],
        "ddamg_hip_solve_squared_chrono_device": [vp, vp, vp, dp, dp, ctypes.c_double, ip, ip, dp],
        "ddamg_hip_vec_upload_parity_device": [vp, vp, ctypes.c_int, dp, ctypes.c_int],
        "ddamg_hip_vec_download_parity_device": [vp, vp, ctypes.c_int, dp],
        "ddamg_hip_schur_apply": [vp, vp, vp, ctypes.c_int],
        "ddamg_hip_schur_apply_device": [vp, dp, dp, ctypes.c_int],
        "ddamg_hip_solve_schur_vec": [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_double, ip, ip, dp],
        "ddamg_hip_solve_schur_device": [vp, ctypes.c_int, ctypes.c_int, dp, dp, dp, ctypes.c_double, ip, ip, dp],
        "ddamg_hip_solve_schur_squared_vec": [vp, vp, vp, ctypes.c_double, ip, ip, dp],
        "ddamg_hip_solve_schur_squared_device": [vp, dp, dp, dp, ctypes.c_double, ip, ip, dp],
        "ddamg_hip_solve_schur_multishift_device": [vp, ctypes.c_int, dp, dp, ctypes.POINTER(dp), ctypes.POINTER(dp), dp, ctypes.c_int, ip, dp, dp],
        "ddamg_hip_solve_schur_multishift_vec": [vp, ctypes.c_int, dp, dp, ctypes.POINTER(vp), vp, ctypes.c_int, ip, dp, dp],
        "ddamg_hip_schur_odd_part_device": [vp, ctypes.c_int, dp, dp],
        "ddamg_hip_multishift_update_time": [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)],
        "ddamg_hip_clover_logdet": [vp, ctypes.c_int, dp, ip],
        "ddamg_hip_force_bilinear_vec": [vp, dp, vp, vp, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_bilinear_device": [vp, dp, dp, dp, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_logdet": [vp, dp, ctypes.c_int, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_bilinear_vec_grid": [vp, dp, vp, vp, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_bilinear_device_grid": [vp, dp, dp, dp, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_logdet_grid": [vp, dp, ctypes.c_int, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_bilinear_multi_vec": [vp, dp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), dp, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_bilinear_multi_device": [vp, dp, ctypes.c_int, ctypes.POINTER(dp), ctypes.POINTER(dp), dp, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_bilinear_multi_vec_grid": [vp, dp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), dp, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_bilinear_multi_device_grid": [vp, dp, ctypes.c_int, ctypes.POINTER(dp), ctypes.POINTER(dp), dp, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_rational_device": [vp, dp, ctypes.c_int, dp, ctypes.POINTER(dp), ctypes.POINTER(dp), ctypes.c_double, ctypes.c_int],
        "ddamg_hip_force_rational_device_grid": [vp, dp, ctypes.c_int, dp, ctypes.POINTER(dp), ctypes.POINTER(dp), ctypes.c_double, ctypes.c_int],
        "ddamg_hip_gauge_loops_device": [vp, dp, dp, dp],
        "ddamg_hip_gauge_force_device": [vp, dp, dp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_links_update_device": [vp, dp, dp, ctypes.c_double],
        "ddamg_hip_links_reunitarize_device": [vp, dp, dp],
        "ddamg_hip_momentum_update_device": [vp, dp, dp, ctypes.c_double],
        "ddamg_hip_momentum_kinetic_device": [vp, dp, dp],
        "ddamg_hip_gauge_loops_device_grid": [vp, dp, dp, dp],
        "ddamg_hip_gauge_force_device_grid": [vp, dp, dp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int],
        "ddamg_hip_links_update_device_grid": [vp, dp, dp, ctypes.c_double],
        "ddamg_hip_links_reunitarize_device_grid": [vp, dp, dp],
        "ddamg_hip_momentum_update_device_grid": [vp, dp, dp, ctypes.c_double],
        "ddamg_hip_momentum_kinetic_device_grid": [vp, dp, dp],
        "ddamg_hip_preconditioner": [vp, dp, dp],
        "ddamg_hip_residual_history": [vp, dp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_get_site_order": [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_rccl_unique_id": [vp],
        "ddamg_hip_comm_init_rccl": [vp, vp],
        "ddamg_hip_comm_init_host": [vp, EXCHANGE_FN, ALLREDUCE_FN, vp],
        "ddamg_hip_halo_plan": [ctypes.POINTER(ctypes.c_int)] * 3 + [ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 3,
        "ddamg_hip_timer_begin": [vp],
        "ddamg_hip_timer_end": [vp, ctypes.POINTER(ctypes.c_float)],
        "ddamg_hip_sync": [vp],
        "ddamg_hip_link_reals": [vp, ctypes.POINTER(ctypes.c_int)],
        "ddamg_hip_memory_in_use": [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    _lib = lib
    return lib


def memory_in_use():
    """(device bytes, pinned host bytes) the library's own buffers hold right now, over all contexts of this process"""
    dev = ctypes.c_size_t(0); pin = ctypes.c_size_t(0)
    load_library().ddamg_hip_memory_in_use(ctypes.byref(dev), ctypes.byref(pin))
    return dev.value, pin.value


class VectorHeader(ctypes.Structure):
    """mirror of ddamg_hip_vector_header (include/ddamg_hip_io.h)"""
    _fields_ = [("vector_type", ctypes.c_char_p), ("m0", ctypes.c_double), ("csw", ctypes.c_double), ("clov_plaq", ctypes.c_double),
                ("hopp_plaq", ctypes.c_double), ("clov_conf_name", ctypes.c_char_p), ("hopp_conf_name", ctypes.c_char_p),
                ("has_eigenvalues", ctypes.c_int), ("eigenvalues", ctypes.POINTER(ctypes.c_double))]


class LimeInfo(ctypes.Structure):
    """mirror of struct ddamg_hip_lime_info (include/ddamg_hip_io.h)"""
    _fields_ = [("kind", ctypes.c_int), ("precision", ctypes.c_int), ("lattice", ctypes.c_int * 4), ("has_plaquette", ctypes.c_int),
                ("plaquette", ctypes.c_double), ("data_offset", ctypes.c_longlong), ("data_length", ctypes.c_longlong),
                ("num_records", ctypes.c_int)]


def _io():
    lib = load_library()
    if not getattr(lib, "_io_ready", False):
        ip = ctypes.POINTER(ctypes.c_int); dp = ctypes.POINTER(ctypes.c_double); cs = ctypes.c_char_p
        lib.ddamg_hip_io_last_error.restype = ctypes.c_char_p
        lib.ddamg_hip_conf_info.argtypes = [cs, ctypes.c_int, ip, dp]
        lib.ddamg_hip_read_conf.argtypes = [cs, ip, ip, ip, ctypes.c_int, dp, dp]
        lib.ddamg_hip_write_conf.argtypes = [cs, ip, ip, ip, ctypes.c_int, dp, ctypes.c_double]
        lib.ddamg_hip_read_conf_multi.argtypes = [cs, ip, ip, ip, ctypes.c_int, dp, dp]
        lib.ddamg_hip_write_conf_multi.argtypes = [cs, ip, ip, ip, ctypes.c_int, dp, ctypes.c_double]
        lib.ddamg_hip_read_vectors.argtypes = [cs, ip, ip, ip, ctypes.c_int, ctypes.c_int, dp]
        lib.ddamg_hip_write_vectors.argtypes = [cs, ip, ip, ip, ctypes.c_int, ctypes.c_int, ctypes.POINTER(VectorHeader), dp]
        lib.ddamg_hip_lime_info.argtypes = [cs, ctypes.POINTER(LimeInfo)]
        lib.ddamg_hip_read_ildg_conf.argtypes = [cs, ip, ip, ip, dp, dp, ip]
        lib.ddamg_hip_write_ildg_conf.argtypes = [cs, ip, ip, ip, ctypes.c_int, dp, ctypes.c_double]
        lib.ddamg_hip_read_lime_vector.argtypes = [cs, ip, ip, ip, dp]
        lib.ddamg_hip_write_lime_vector.argtypes = [cs, ip, ip, ip, ctypes.POINTER(VectorHeader), dp]
        lib._io_ready = True
    return lib


def _io_check(rc):
    if rc != 0:
        raise DDAMGError(_io().ddamg_hip_io_last_error().decode())


def _i4(v):
    return (ctypes.c_int * 4)(*[int(x) for x in v])


def conf_info(path, big_endian=False):
    """(lattice [T,Z,Y,X], plaquette) stored in a configuration file of the reference's format (src/io.c:489-507)"""
    L = (ctypes.c_int * 4)(); plaq = ctypes.c_double(0)
    _io_check(_io().ddamg_hip_conf_info(os.fsencode(path), int(big_endian), L, ctypes.byref(plaq)))
    return list(L), plaq.value


def read_conf(path, global_lattice, process_grid=(1, 1, 1, 1), process_coords=(0, 0, 0, 0), big_endian=False):
    """this process's part of a configuration file: ([V_local][4][9][2] links, plaquette of the header)"""
    Vloc = int(np.prod([g // max(p, 1) for g, p in zip(global_lattice, process_grid)]))
    out = np.zeros((Vloc, 4, 9, 2)); plaq = ctypes.c_double(0)
    _io_check(_io().ddamg_hip_read_conf(os.fsencode(path), _i4(global_lattice), _i4(process_grid), _i4(process_coords), int(big_endian), _dp(out), ctypes.byref(plaq)))
    return out, plaq.value


def write_conf(path, global_lattice, gauge_local, plaq, process_grid=(1, 1, 1, 1), process_coords=(0, 0, 0, 0), big_endian=False):
    a = np.ascontiguousarray(gauge_local, dtype=np.float64)
    _io_check(_io().ddamg_hip_write_conf(os.fsencode(path), _i4(global_lattice), _i4(process_grid), _i4(process_coords), int(big_endian), _dp(a), float(plaq)))


def read_conf_multi(base, global_lattice, process_grid, process_coords, big_endian=False):
    """this process's file of a multi-file configuration (read_conf_multi, src/io.c:566-668): <base>.pt<T>pz<Z>py<Y>px<X>"""
    Vloc = int(np.prod([g // max(p, 1) for g, p in zip(global_lattice, process_grid)]))
    out = np.zeros((Vloc, 4, 9, 2)); plaq = ctypes.c_double(0)
    _io_check(_io().ddamg_hip_read_conf_multi(os.fsencode(base), _i4(global_lattice), _i4(process_grid), _i4(process_coords), int(big_endian), _dp(out), ctypes.byref(plaq)))
    return out, plaq.value


def write_conf_multi(base, global_lattice, gauge_local, plaq, process_grid, process_coords, big_endian=False):
    a = np.ascontiguousarray(gauge_local, dtype=np.float64)
    _io_check(_io().ddamg_hip_write_conf_multi(os.fsencode(base), _i4(global_lattice), _i4(process_grid), _i4(process_coords), int(big_endian), _dp(a), float(plaq)))


def read_vectors(path, global_lattice, n=1, process_grid=(1, 1, 1, 1), process_coords=(0, 0, 0, 0), big_endian=False):
    """n spinors ([n][V_local][12][2]) from a vector / test-vector file of the reference (src/io.c:704-846, 951-1124)"""
    Vloc = int(np.prod([g // max(p, 1) for g, p in zip(global_lattice, process_grid)]))
    out = np.zeros((n, Vloc, 12, 2))
    _io_check(_io().ddamg_hip_read_vectors(os.fsencode(path), _i4(global_lattice), _i4(process_grid), _i4(process_coords), int(n), int(big_endian), _dp(out)))
    return out


def write_vectors(path, global_lattice, vectors_local, header=None, process_grid=(1, 1, 1, 1), process_coords=(0, 0, 0, 0), big_endian=False):
    """header: None (bare data, one spinor) or a dict with the fields of write_header (src/io.c:671-702):
    vector_type, m0, csw, clov_plaq, hopp_plaq, clov_conf_name, hopp_conf_name, eigenvalues"""
    a = np.ascontiguousarray(vectors_local, dtype=np.float64)
    Vloc = int(np.prod([g // max(p, 1) for g, p in zip(global_lattice, process_grid)]))
    if a.size % (Vloc * 24):
        raise DDAMGError("write_vectors: expected [n][V_local][12] complex numbers")
    n = a.size // (Vloc * 24)
    hp = None
    if header is not None:
        h, _keep = _vector_header(header)
        hp = ctypes.byref(h)
    _io_check(_io().ddamg_hip_write_vectors(os.fsencode(path), _i4(global_lattice), _i4(process_grid), _i4(process_coords), n, int(big_endian), hp, _dp(a)))


def _vector_header(header):
    """(ddamg_hip_vector_header, what it points into) from the dict write_vectors documents"""
    ev = header.get("eigenvalues")
    evbuf = np.ascontiguousarray(ev, dtype=np.float64) if ev is not None else None
    h = VectorHeader(str(header.get("vector_type", "")).encode(), float(header.get("m0", 0)), float(header.get("csw", 0)),
                     float(header.get("clov_plaq", 0)), float(header.get("hopp_plaq", 0)), str(header.get("clov_conf_name", "")).encode(),
                     str(header.get("hopp_conf_name", "")).encode(), int(ev is not None), _dp(evbuf) if evbuf is not None else None)
    return h, evbuf


LIME_KINDS = {0: None, 1: "gauge", 2: "vector"}


def lime_info(path):
    """what the record headers of a LIME file say (include/ddamg_hip_io.h): dict with kind (None, "gauge", "vector"), precision,
    lattice [T,Z,Y,X], has_plaquette, plaquette (the file's number, in [0,1]), data_offset, data_length, num_records"""
    info = LimeInfo()
    _io_check(_io().ddamg_hip_lime_info(os.fsencode(path), ctypes.byref(info)))
    return dict(kind=LIME_KINDS[info.kind], precision=info.precision, lattice=list(info.lattice), has_plaquette=bool(info.has_plaquette),
                plaquette=info.plaquette, data_offset=info.data_offset, data_length=info.data_length, num_records=info.num_records)


def read_ildg_conf(path, global_lattice, process_grid=(1, 1, 1, 1), process_coords=(0, 0, 0, 0), out=None):
    """this process's part of an ILDG configuration (fp64 or fp32 file): ([V_local][4][9][2] links in the order T,Z,Y,X, plaquette
    in [0,3] or None if the file has none); `out` takes the links instead of a fresh array"""
    Vloc = int(np.prod([g // max(p, 1) for g, p in zip(global_lattice, process_grid)]))
    if out is None:
        out = np.zeros((Vloc, 4, 9, 2))
    if out.dtype != np.float64 or not out.flags.c_contiguous or out.size != Vloc * 72:
        raise DDAMGError("read_ildg_conf: `out` must be a C-contiguous float64 array of V_local*4*9 complex numbers")
    plaq = ctypes.c_double(0); has = ctypes.c_int(0)
    _io_check(_io().ddamg_hip_read_ildg_conf(os.fsencode(path), _i4(global_lattice), _i4(process_grid), _i4(process_coords), _dp(out),
                                             ctypes.byref(plaq), ctypes.byref(has)))
    return out, (plaq.value if has.value else None)


def write_ildg_conf(path, global_lattice, gauge_local, plaq, process_grid=(1, 1, 1, 1), process_coords=(0, 0, 0, 0), precision=64):
    """plaq in [0,3], as set_gauge returns it; the file carries plaq / 3"""
    a = np.ascontiguousarray(gauge_local, dtype=np.float64)
    _io_check(_io().ddamg_hip_write_ildg_conf(os.fsencode(path), _i4(global_lattice), _i4(process_grid), _i4(process_coords), int(precision), _dp(a), float(plaq)))


def read_lime_vector(path, global_lattice, process_grid=(1, 1, 1, 1), process_coords=(0, 0, 0, 0), out=None):
    """this process's part ([V_local][12][2]) of the spinor of a SciDAC/ETMC LIME file (fp64 or fp32)"""
    Vloc = int(np.prod([g // max(p, 1) for g, p in zip(global_lattice, process_grid)]))
    if out is None:
        out = np.zeros((Vloc, 12, 2))
    if out.dtype != np.float64 or not out.flags.c_contiguous or out.size != Vloc * 24:
        raise DDAMGError("read_lime_vector: `out` must be a C-contiguous float64 array of V_local*12 complex numbers")
    _io_check(_io().ddamg_hip_read_lime_vector(os.fsencode(path), _i4(global_lattice), _i4(process_grid), _i4(process_coords), _dp(out)))
    return out


def write_lime_vector(path, global_lattice, vector_local, header=None, process_grid=(1, 1, 1, 1), process_coords=(0, 0, 0, 0)):
    """one spinor as the reference's four records (lime_write_info, src/lime_io.c:163-217); header: the dict of write_vectors"""
    a = np.ascontiguousarray(vector_local, dtype=np.float64)
    Vloc = int(np.prod([g // max(p, 1) for g, p in zip(global_lattice, process_grid)]))
    if a.size != Vloc * 24:
        raise DDAMGError("write_lime_vector: expected [V_local][12] complex numbers")
    h, _keep = _vector_header(header) if header is not None else (None, None)
    _io_check(_io().ddamg_hip_write_lime_vector(os.fsencode(path), _i4(global_lattice), _i4(process_grid), _i4(process_coords),
                                                ctypes.byref(h) if h is not None else None, _dp(a)))


def _check(rc):
    if rc != 0:
        raise DDAMGError(load_library().ddamg_hip_last_error().decode())


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _dev(a, reals, what):
    """the address of an array of `reals` float64 numbers in device memory: an integer address (the caller vouches for size and
    type; the library checks that it is device memory) or any object with data_ptr().  A torch tensor is checked for dtype,
    contiguity, element count and is_cuda, and its device's current stream is waited for, because the library works on a stream
    of its own."""
    if isinstance(a, int):
        return ctypes.cast(ctypes.c_void_p(a), ctypes.POINTER(ctypes.c_double))
    if not hasattr(a, "data_ptr"):
        raise DDAMGError(f"{what}: expected an integer device address or an object with data_ptr(), got {type(a).__name__}")
    if hasattr(a, "is_cuda"):   # a torch tensor
        import torch
        if not a.is_cuda:
            raise DDAMGError(f"{what}: the tensor is in host memory (host arrays go through the call without _device)")
        if a.dtype != torch.float64:
            raise DDAMGError(f"{what}: the tensor must be float64, got {a.dtype}")
        if not a.is_contiguous():
            raise DDAMGError(f"{what}: the tensor must be contiguous")
        if a.numel() != reals:
            raise DDAMGError(f"{what}: expected {reals} reals, got {a.numel()}")
        torch.cuda.current_stream(a.device).synchronize()
    return ctypes.cast(ctypes.c_void_p(int(a.data_ptr())), ctypes.POINTER(ctypes.c_double))


def _dev_raw(a, what):
    """the address of raw bytes in device memory (the library checks device, size and alignment): an integer address, or an object
    with data_ptr() -- a torch tensor of any dtype, which must be contiguous and on the device, and whose stream is waited for"""
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    if not hasattr(a, "data_ptr"):
        raise DDAMGError(f"{what}: expected an integer device address or an object with data_ptr(), got {type(a).__name__}")
    if hasattr(a, "is_cuda"):
        import torch
        if not a.is_cuda:
            raise DDAMGError(f"{what}: the tensor is in host memory")
        if not a.is_contiguous():
            raise DDAMGError(f"{what}: the tensor must be contiguous")
        torch.cuda.current_stream(a.device).synchronize()
    return ctypes.c_void_p(int(a.data_ptr()))


def default_params():
    p = Params()
    load_library().ddamg_hip_default_params(ctypes.byref(p))
    return p


class Vector:
    def __init__(self, ctx, level, precision):
        self.ctx, self.level, self.precision = ctx, level, precision
        self.ndof = ctx.ndof(level)
        self.V = ctx.volume(level)
        self._h = ctypes.c_void_p()
        _check(ctx._lib.ddamg_hip_vec_create(ctx._h, level, precision, ctypes.byref(self._h)))

    def upload(self, host_lex):
        a = np.ascontiguousarray(host_lex, dtype=np.float64)
        if a.size != self.V * self.ndof * 2:
            raise DDAMGError(f"vector upload: expected {self.V * self.ndof * 2} reals, got {a.size}")
        _check(self.ctx._lib.ddamg_hip_vec_upload(self.ctx._h, self._h, _dp(a)))
        return self

    def download(self):
        out = np.empty((self.V, self.ndof, 2), dtype=np.float64)
        _check(self.ctx._lib.ddamg_hip_vec_download(self.ctx._h, self._h, _dp(out)))
        return out

    def upload_device(self, dev_lex):
        """upload from a lexicographic float64 array in device memory (integer address or an object with data_ptr())"""
        _check(self.ctx._lib.ddamg_hip_vec_upload_device(self.ctx._h, self._h, _dev(dev_lex, self.V * self.ndof * 2, "upload_device")))
        return self

    def download_device(self, dev_lex):
        """download into a lexicographic float64 array in device memory; returns dev_lex"""
        _check(self.ctx._lib.ddamg_hip_vec_download_device(self.ctx._h, self._h, _dev(dev_lex, self.V * self.ndof * 2, "download_device")))
        return dev_lex

    def upload_parity_device(self, parity, half_dev, zero_other=True):
        """the sites of `parity` (0 even, 1 odd) from a half field in device memory ([V/2][12] complex float64, half index =
        lexicographic index >> 1); zero_other: the other parity becomes zero, else it is left alone"""
        _check(self.ctx._lib.ddamg_hip_vec_upload_parity_device(self.ctx._h, self._h, int(parity), _dev(half_dev, self.V * self.ndof, "upload_parity_device"),
                                                                int(bool(zero_other))))
        return self

    def download_parity_device(self, parity, half_dev):
        """the sites of `parity` into a half field in device memory; returns half_dev"""
        _check(self.ctx._lib.ddamg_hip_vec_download_parity_device(self.ctx._h, self._h, int(parity), _dev(half_dev, self.V * self.ndof, "download_parity_device")))
        return half_dev

    def free(self):
        if self._h:
            self.ctx._lib.ddamg_hip_vec_destroy(self.ctx._h, self._h)
            self._h = ctypes.c_void_p()


class Chrono:
    """Mirror of ddamg_hip_chrono: the last `depth` solutions of a context, for the guess of the next solve; freed before the context"""

    def __init__(self, ctx, depth):
        self.ctx, self.depth = ctx, depth
        self._h = ctypes.c_void_p()
        _check(ctx._lib.ddamg_hip_chrono_create(ctx._h, int(depth), ctypes.byref(self._h)))

    def push(self, x):
        self.ctx.chrono_push_vec(self, x)

    def guess(self, x0, b, system=0):
        return self.ctx.chrono_guess_vec(self, x0, b, system)

    def reset(self):
        self.ctx.chrono_reset(self)

    def count(self):
        return self.ctx.chrono_count(self)

    def free(self):
        if self._h:
            _check(self.ctx._lib.ddamg_hip_chrono_destroy(self.ctx._h, self._h))
            self._h = ctypes.c_void_p()


class Context:
    """Mirror of ddamg_hip_ctx; one per process and GPU."""

    def __init__(self, params):
        self._lib = load_library()
        self.params = params
        self._h = ctypes.c_void_p()
        _check(self._lib.ddamg_hip_create(ctypes.byref(params), ctypes.byref(self._h)))

    def volume(self, level=0):
        return int(np.prod(list(self.params.local_lattice[level])))

    def ndof(self, level=0):
        return 12 if level == 0 else 2 * self.params.num_vect[level - 1]

    def set_gauge(self, gauge_lex, anti_pbc=True):
        a = np.ascontiguousarray(gauge_lex, dtype=np.float64)
        if a.size != self.volume(0) * 72:
            raise DDAMGError("set_gauge: gauge field must hold V*4*9 complex numbers")
        plaq = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_set_gauge(self._h, _dp(a), int(bool(anti_pbc)), ctypes.byref(plaq)))
        return plaq.value

    def set_gauge2(self, hopp_gauge_lex, clover_gauge_lex, anti_pbc=False):
        """hopping term from the first field, clover term and plaquette from the second (open boundaries)"""
        a = np.ascontiguousarray(hopp_gauge_lex, dtype=np.float64); b = np.ascontiguousarray(clover_gauge_lex, dtype=np.float64)
        if a.size != self.volume(0) * 72 or b.size != a.size:
            raise DDAMGError("set_gauge2: both gauge fields must hold V*4*9 complex numbers")
        plaq = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_set_gauge2(self._h, _dp(a), _dp(b), int(bool(anti_pbc)), ctypes.byref(plaq)))
        return plaq.value

    def set_gauge_device(self, gauge_dev_lex, anti_pbc=True):
        """set_gauge from links in device memory ([V][4][9] complex float64, lexicographic): an integer address or an object
        with data_ptr(), a torch tensor for instance; the array is not written"""
        plaq = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_set_gauge_device(self._h, _dev(gauge_dev_lex, self.volume(0) * 72, "set_gauge_device"), int(bool(anti_pbc)),
                                                    ctypes.byref(plaq)))
        return plaq.value

    def set_gauge2_device(self, hopp_gauge_dev_lex, clover_gauge_dev_lex, anti_pbc=False):
        """set_gauge2 from two fields in device memory"""
        plaq = ctypes.c_double(0)
        n = self.volume(0) * 72
        _check(self._lib.ddamg_hip_set_gauge2_device(self._h, _dev(hopp_gauge_dev_lex, n, "set_gauge2_device"),
                                                     _dev(clover_gauge_dev_lex, n, "set_gauge2_device"), int(bool(anti_pbc)), ctypes.byref(plaq)))
        return plaq.value

    def set_gauge_device_grid(self, gauge_dev_lex, anti_pbc=True):
        """set_gauge_device on any process grid: this process's links in device memory, the neighbours' one-site shell exchanged
        device to device over the installed transport.  Collective: every process of the grid calls it.  Returns the global
        plaquette.  On an undivided context it is set_gauge_device."""
        plaq = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_set_gauge_device_grid(self._h, _dev(gauge_dev_lex, self.volume(0) * 72, "set_gauge_device_grid"), int(bool(anti_pbc)),
                                                         ctypes.byref(plaq)))
        return plaq.value

    def set_gauge2_device_grid(self, hopp_gauge_dev_lex, clover_gauge_dev_lex, anti_pbc=False):
        """set_gauge2_device on any process grid (collective); only the clover field's shell travels"""
        plaq = ctypes.c_double(0)
        n = self.volume(0) * 72
        _check(self._lib.ddamg_hip_set_gauge2_device_grid(self._h, _dev(hopp_gauge_dev_lex, n, "set_gauge2_device_grid"),
                                                          _dev(clover_gauge_dev_lex, n, "set_gauge2_device_grid"), int(bool(anti_pbc)), ctypes.byref(plaq)))
        return plaq.value

    def load_ildg_conf(self, path, anti_pbc=True):
        """the configuration of an ILDG file becomes the operator (file -> pinned staging -> device links -> operator; on a process
        grid every process reads its own part that way and the neighbours' shell of links travels device to device, as in
        set_gauge_device_grid: collective, a transport must be installed).  Returns (plaquette computed from the links, the file's plaquette
        times three or None if it has none), both in [0,3]"""
        plaq = ctypes.c_double(0); fplaq = ctypes.c_double(0); has = ctypes.c_int(0)
        _check(self._lib.ddamg_hip_load_ildg_conf(self._h, os.fsencode(path), int(bool(anti_pbc)), ctypes.byref(plaq), ctypes.byref(fplaq),
                                                  ctypes.byref(has)))
        return plaq.value, (fplaq.value if has.value else None)

    def ildg_to_links_device(self, raw_dev, precision, nsites, links_dev):
        """the data of an ildg-binary-data record in device memory (big-endian, fp64 or fp32, directions X,Y,Z,T) -> links
        [nsites][4][9] complex float64 as set_gauge_device takes them; returns links_dev"""
        _check(self._lib.ddamg_hip_ildg_to_links_device(self._h, _dev_raw(raw_dev, "ildg_to_links_device"), int(precision), int(nsites),
                                                        _dev(links_dev, int(nsites) * 72, "ildg_to_links_device")))
        return links_dev

    def links_to_ildg_device(self, links_dev, precision, nsites, raw_dev):
        """the inverse: links in device memory -> the bytes of an ildg-binary-data record (fp32: rounded to nearest); returns raw_dev"""
        _check(self._lib.ddamg_hip_links_to_ildg_device(self._h, _dev(links_dev, int(nsites) * 72, "links_to_ildg_device"), int(precision), int(nsites),
                                                        _dev_raw(raw_dev, "links_to_ildg_device")))
        return raw_dev

    def clover_kernel_time(self, gauge_dev_lex, which, reps=10):
        """(milliseconds per launch, plaquette) of the field-strength kernel (which = 0), the host path's clover kernel (1), the
        field-strength, assembly and plaquette-sum kernels together (2) or, on a process grid, the field-strength kernel on the
        extended lattice (3) on links in device memory; a measurement"""
        ms = ctypes.c_float(0); plaq = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_clover_kernel_time(self._h, _dev(gauge_dev_lex, self.volume(0) * 72, "clover_kernel_time"), int(which), int(reps),
                                                      ctypes.byref(ms), ctypes.byref(plaq)))
        return ms.value, plaq.value

    def set_operator(self, D_lex, clover_lex):
        D = np.ascontiguousarray(D_lex, dtype=np.float64)
        cl = np.ascontiguousarray(clover_lex, dtype=np.float64)
        V = self.volume(0)
        if D.size != V * 72 or cl.size != V * 84:
            raise DDAMGError("set_operator: D must be [V][36] complex and clover [V][42] complex")
        _check(self._lib.ddamg_hip_set_operator(self._h, _dp(D), _dp(cl)))

    def shift_mass(self, m0):
        """shift_update of the reference: change the mass of the operator that is set, on the device, on every level"""
        _check(self._lib.ddamg_hip_shift_mass(self._h, float(m0)))

    def scale_clover(self, scale_even, scale_odd):
        """clover term times scale_even / scale_odd by global parity, on the device (absolute: (1, 1) restores the operator)"""
        _check(self._lib.ddamg_hip_scale_clover(self._h, float(scale_even), float(scale_odd)))

    def get_operator(self):
        V = self.volume(0)
        D = np.empty((V, 36, 2)); cl = np.empty((V, 42, 2))
        _check(self._lib.ddamg_hip_get_operator(self._h, _dp(D), _dp(cl)))
        return D, cl

    def link_reals(self):
        """reals per link that the fp32 fine operator reads: 18 (full links), 12 (two-row form) or 10 (pivot form)"""
        n = ctypes.c_int(0)
        _check(self._lib.ddamg_hip_link_reals(self._h, ctypes.byref(n)))
        return n.value

    def vector(self, level=0, precision=32):
        return Vector(self, level, precision)

    def dirac_apply(self, out, inp):
        _check(self._lib.ddamg_hip_dirac_apply(self._h, out._h, inp._h))

    def dirac_apply_dagger(self, out, inp):
        """out = D^dagger inp = gamma5 D gamma5 inp in one pass (fine-level Vectors of one precision, out is not inp)"""
        _check(self._lib.ddamg_hip_dirac_apply_dagger(self._h, out._h, inp._h))

    def gamma5(self, out, inp):
        """out = gamma5 inp: spin components 0 and 1 change sign (fine-level Vectors of one precision; out may be inp)"""
        _check(self._lib.ddamg_hip_gamma5(self._h, out._h, inp._h))

    # ---- BLAS-1 ----
    def vec_copy(self, dst, src):
        _check(self._lib.ddamg_hip_vec_copy(self._h, dst._h, src._h))

    def vec_axpy(self, z, x, y, alpha):
        alpha = complex(alpha)
        _check(self._lib.ddamg_hip_vec_axpy(self._h, z._h, x._h, y._h, alpha.real, alpha.imag))

    def vec_dot(self, x, y):
        """returns (<x,y>, ||x||)"""
        re = ctypes.c_double(0); im = ctypes.c_double(0); nx = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_vec_dot(self._h, x._h, y._h, ctypes.byref(re), ctypes.byref(im), ctypes.byref(nx)))
        return complex(re.value, im.value), nx.value

    # ---- multigrid ----
    def vprec(self):
        return 64 if self.params.mixed_precision == 0 else 32

    def setup(self, setup_iterations=-1):
        ci = ctypes.c_int(0)
        _check(self._lib.ddamg_hip_setup(self._h, int(setup_iterations), ctypes.byref(ci)))
        return ci.value

    def setup_update(self, iterations):
        ci = ctypes.c_int(0)
        _check(self._lib.ddamg_hip_setup_update(self._h, int(iterations), ctypes.byref(ci)))
        return ci.value

    def set_test_vectors(self, tv_lex, orthonormalised=False):
        a = np.ascontiguousarray(tv_lex, dtype=np.float64)
        if a.size != self.params.num_vect[0] * self.volume(0) * 24:
            raise DDAMGError("set_test_vectors: expected [num_vect][V][12] complex numbers")
        _check(self._lib.ddamg_hip_set_test_vectors(self._h, _dp(a), int(bool(orthonormalised))))

    def get_interpolation(self):
        out = np.empty((self.params.num_vect[0], self.volume(0), 12, 2))
        _check(self._lib.ddamg_hip_get_interpolation(self._h, _dp(out)))
        return out

    def get_test_vectors(self):
        out = np.zeros((self.params.num_vect[0], self.volume(0), 12, 2))
        _check(self._lib.ddamg_hip_get_test_vectors(self._h, _dp(out)))
        return out

    def get_coarse_operator(self, level=1):
        n = self.ndof(level); Vc = self.volume(level)
        D = np.empty((Vc, 4, n * n, 2)); cl = np.empty((Vc, n * (n + 1) // 2, 2))
        _check(self._lib.ddamg_hip_get_coarse_operator_level(self._h, int(level), _dp(D), _dp(cl)))
        return D, cl

    def set_coarse_operator(self, D, cl, level=1):
        n = self.ndof(level); Vc = self.volume(level)
        D = np.ascontiguousarray(D, dtype=np.float64); cl = np.ascontiguousarray(cl, dtype=np.float64)
        if D.size != Vc * 4 * n * n * 2 or cl.size != Vc * n * (n + 1):
            raise DDAMGError("set_coarse_operator: wrong array sizes")
        _check(self._lib.ddamg_hip_set_coarse_operator_level(self._h, int(level), _dp(D), _dp(cl)))

    def set_interpolation(self, P_lex, level=0):
        """interpolation vectors of `level` as they are ([num_vect][V][ndof][2], lexicographic sites of that level); builds the
        operator of level + 1 and runs the initial setup of the levels below"""
        P = np.ascontiguousarray(P_lex, dtype=np.float64)
        if P.size != self.params.num_vect[level] * self.volume(level) * self.ndof(level) * 2:
            raise DDAMGError("set_interpolation: wrong array size")
        _check(self._lib.ddamg_hip_set_interpolation_level(self._h, int(level), _dp(P)))

    def kcycle(self, x, b):
        it = ctypes.c_int(0)
        _check(self._lib.ddamg_hip_kcycle(self._h, x._h, b._h, ctypes.byref(it)))
        return it.value

    def _many(self, fn, outs, ins, *extra):
        n = len(ins)
        VP = ctypes.c_void_p * n
        _check(fn(self._h, n, VP(*[v._h for v in outs]), VP(*[v._h for v in ins]), *extra))

    def coarse_apply_many(self, outs, ins):
        """the coarse operator of the vectors' level for up to 32 right-hand sides at once (matrix cores)"""
        self._many(self._lib.ddamg_hip_coarse_apply_many, outs, ins)

    def smoother_many(self, phis, etas, cycles, initial_guess_zero=True):
        self._many(self._lib.ddamg_hip_smoother_many, phis, etas, int(cycles), int(bool(initial_guess_zero)))

    def vcycle_many(self, phis, etas):
        self._many(self._lib.ddamg_hip_vcycle_many, phis, etas)

    def kcycle_many(self, xs, bs):
        its = (ctypes.c_int * len(bs))()
        self._many(self._lib.ddamg_hip_kcycle_many, xs, bs, its)
        return list(its)

    def smoother(self, phi, eta, cycles, initial_guess_zero=True):
        _check(self._lib.ddamg_hip_smoother(self._h, phi._h, eta._h, int(cycles), int(bool(initial_guess_zero))))

    def restrict(self, coarse, fine):
        _check(self._lib.ddamg_hip_restrict(self._h, coarse._h, fine._h))

    def interpolate(self, fine, coarse, add=False):
        _check(self._lib.ddamg_hip_interpolate(self._h, fine._h, coarse._h, int(bool(add))))

    def coarse_apply(self, out, inp):
        _check(self._lib.ddamg_hip_coarse_apply(self._h, out._h, inp._h))

    def coarse_solve(self, x, b):
        it = ctypes.c_int(0)
        _check(self._lib.ddamg_hip_coarse_solve(self._h, x._h, b._h, ctypes.byref(it)))
        return it.value

    def set_coarse_storage(self, bits):
        """storage of the coarsest couplings for the solve: 32 (default) or 16 (fp16 pairs + one fp32 scale per matrix, fp32
        accumulation); raises DDAMGError where the context cannot carry 16 (see include/ddamg_hip.h)"""
        _check(self._lib.ddamg_hip_set_coarse_storage(self._h, int(bits)))

    def set_transfer_storage(self, bits):
        """storage of the fine level's interpolation operator for the solve: 32 (default) or 16 (fp16 entries + one fp32 scale per
        aggregate, vector and chirality, fp32 accumulation); raises DDAMGError where the context cannot carry 16 (see
        include/ddamg_hip.h)"""
        _check(self._lib.ddamg_hip_set_transfer_storage(self._h, int(bits)))

    def set_intermediate_storage(self, bits):
        """storage of the couplings of every intermediate level for the solve: 32 (default) or 16 (fp16 pairs + one fp32 scale per
        matrix, fp32 accumulation); raises DDAMGError where the context cannot carry 16 (see include/ddamg_hip.h)"""
        _check(self._lib.ddamg_hip_set_intermediate_storage(self._h, int(bits)))

    def coarse_hop(self, out, inp, parity, sign=1.0, accumulate=False):
        """a half hopping term of the coarsest level: out (+)= sign * hopping terms of inp on the even (0) / odd (1) sites"""
        _check(self._lib.ddamg_hip_coarse_hop(self._h, out._h, inp._h, int(parity), float(sign), int(bool(accumulate))))

    def coarse_self_mul(self, out, inp, parity, inverse=False):
        """out = M0 inp (or M0^-1 inp) on the even (0) / odd (1) sites of the coarsest level"""
        _check(self._lib.ddamg_hip_coarse_self_mul(self._h, out._h, inp._h, int(parity), int(bool(inverse))))

    def coarse_solve_many(self, xs, bs):
        """the coarsest-level solve for up to 32 right-hand sides in lockstep (matrix-core coarse operator); returns the list of
        iteration counts (-1: the column needs the one-at-a-time solver)"""
        n = len(bs)
        VP = ctypes.c_void_p * n
        its = (ctypes.c_int * n)()
        _check(self._lib.ddamg_hip_coarse_solve_many(self._h, n, VP(*[v._h for v in xs]), VP(*[v._h for v in bs]), its))
        return list(its)

    def vcycle(self, phi, eta):
        _check(self._lib.ddamg_hip_vcycle(self._h, phi._h, eta._h))

    def _solve_host(self, name, b_lex, tol, out, squared=False):
        """a host-array solve entry point `ddamg_hip_<name>`; squared: two iteration counts each, returned as pairs"""
        b = np.ascontiguousarray(b_lex, dtype=np.float64)
        if b.size != self.volume(0) * 24:
            raise DDAMGError(f"{name}: right-hand side must hold V*12 complex numbers")
        x = out if out is not None else np.empty((self.volume(0), 12, 2))
        if x.dtype != np.float64 or not x.flags.c_contiguous or x.size != b.size:
            raise DDAMGError(f"{name}: `out` must be a C-contiguous float64 array of V*12 complex numbers")
        return (x,) + self._solve_call(name, _dp(x), _dp(b), tol, squared)

    def _solve_call(self, name, x, b, tol, squared=False):
        it = (ctypes.c_int * 2)(); ci = (ctypes.c_int * 2)(); rr = ctypes.c_double(0)
        _check(getattr(self._lib, "ddamg_hip_" + name)(self._h, x, b, float(tol), it, ci, ctypes.byref(rr)))
        if squared:
            return (it[0], it[1]), (ci[0], ci[1]), rr.value
        return it[0], ci[0], rr.value

    def _solve_dev(self, name, x_dev_lex, b_dev_lex, tol, squared=False):
        n = self.volume(0) * 24
        return self._solve_call(name, _dev(x_dev_lex, n, name), _dev(b_dev_lex, n, name), tol, squared)

    def solve(self, b_lex, tol=0.0, out=None):
        """returns (x_lex, iterations, coarse_iterations, true relative residual); `out` reuses a solution array (a fresh
        one is first touched page by page while the device writes into it, which costs more than the solve at 32^4)"""
        return self._solve_host("solve", b_lex, tol, out)

    def solve_vec(self, x, b, tol=0.0):
        """device-resident solve: x, b fine-level fp64 Vectors; returns (iterations, coarse_iterations, relres)"""
        return self._solve_call("solve_vec", x._h, b._h, tol)

    # ---- HMC solves: D^dagger x = b as x = gamma5 D^-1 gamma5 b, and D^dagger D x = b as the two solves back to back ----
    def solve_dagger(self, b_lex, tol=0.0, out=None):
        """D^dagger x = b; returns as solve() does (the numbers are those of the solve of D on gamma5 b)"""
        return self._solve_host("solve_dagger", b_lex, tol, out)

    def solve_dagger_vec(self, x, b, tol=0.0):
        return self._solve_call("solve_dagger_vec", x._h, b._h, tol)

    def solve_dagger_device(self, x_dev_lex, b_dev_lex, tol=0.0):
        return self._solve_dev("solve_dagger_device", x_dev_lex, b_dev_lex, tol)

    def solve_squared(self, b_lex, tol=0.0, out=None):
        """D^dagger D x = b; returns (x_lex, (iterations of the D^dagger solve, of the D solve), the same pair of coarse iterations,
        ||b - D^dagger D x|| / ||b||): that residual carries the condition of D^dagger and is not promised to be below tol"""
        return self._solve_host("solve_squared", b_lex, tol, out, squared=True)

    def solve_squared_vec(self, x, b, tol=0.0):
        return self._solve_call("solve_squared_vec", x._h, b._h, tol, squared=True)

    def solve_squared_device(self, x_dev_lex, b_dev_lex, tol=0.0):
        return self._solve_dev("solve_squared_device", x_dev_lex, b_dev_lex, tol, squared=True)

    # ---- solves from a starting vector; the guess extrapolated from past solutions (Chrono) ----
    # system: 0 solves D x = b, 1 solves D^dagger x = b
    def _guess_call(self, name, head, x, b, tol):
        """`ddamg_hip_<name>`(ctx, *head, x, b, tol, ...); returns (iterations, coarse_iterations, relres, guess_relres)"""
        it = ctypes.c_int(0); ci = ctypes.c_int(0); rr = ctypes.c_double(0); gr = ctypes.c_double(0)
        _check(getattr(self._lib, "ddamg_hip_" + name)(self._h, *head, x, b, float(tol), ctypes.byref(it), ctypes.byref(ci), ctypes.byref(rr),
                                                       ctypes.byref(gr)))
        return it.value, ci.value, rr.value, gr.value

    def solve_guess(self, x0_lex, b_lex, tol=0.0, system=0):
        """the solve from the guess x0_lex (not written); returns (x_lex, iterations, coarse_iterations, relres = ||b - A x|| / ||b||,
        guess_relres = ||b - A x0|| / ||b||)"""
        b = np.ascontiguousarray(b_lex, dtype=np.float64)
        x = np.array(x0_lex, dtype=np.float64, order="C")
        if b.size != self.volume(0) * 24 or x.size != b.size:
            raise DDAMGError("solve_guess: guess and right-hand side must hold V*12 complex numbers")
        return (x,) + self._guess_call("solve_guess", (int(system),), _dp(x), _dp(b), tol)

    def solve_guess_vec(self, x, b, tol=0.0, system=0):
        """x: the guess on entry, the solution on return"""
        return self._guess_call("solve_guess_vec", (int(system),), x._h, b._h, tol)

    def solve_guess_device(self, x_dev_lex, b_dev_lex, tol=0.0, system=0):
        n = self.volume(0) * 24
        return self._guess_call("solve_guess_device", (int(system),), _dev(x_dev_lex, n, "solve_guess_device"), _dev(b_dev_lex, n, "solve_guess_device"), tol)

    def chrono_create(self, depth):
        """a store of the last `depth` solutions (1..8): a Chrono"""
        return Chrono(self, depth)

    def chrono_destroy(self, h):
        h.free()

    def chrono_reset(self, h):
        _check(self._lib.ddamg_hip_chrono_reset(self._h, h._h))

    def chrono_count(self, h):
        n = ctypes.c_int(0)
        _check(self._lib.ddamg_hip_chrono_count(self._h, h._h, ctypes.byref(n)))
        return n.value

    def chrono_push_vec(self, h, x):
        _check(self._lib.ddamg_hip_chrono_push_vec(self._h, h._h, x._h))

    def chrono_guess_vec(self, h, x0, b, system=0):
        """x0 = the combination of the stored vectors with the least residual for the operator that is set now; returns (vectors
        that entered it, predicted ||b - A x0|| / ||b||)"""
        kept = ctypes.c_int(0); pr = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_chrono_guess_vec(self._h, h._h, int(system), x0._h, b._h, ctypes.byref(kept), ctypes.byref(pr)))
        return kept.value, pr.value

    def solve_chrono_vec(self, h, x, b, tol=0.0, system=0):
        """guess from the store, solve from it, push the solution; returns as solve_guess_vec"""
        return self._guess_call("solve_chrono_vec", (h._h, int(system)), x._h, b._h, tol)

    def solve_chrono_device(self, h, x_dev_lex, b_dev_lex, tol=0.0, system=0):
        n = self.volume(0) * 24
        return self._guess_call("solve_chrono_device", (h._h, int(system)), _dev(x_dev_lex, n, "solve_chrono_device"),
                                _dev(b_dev_lex, n, "solve_chrono_device"), tol)

    def _squared_chrono_call(self, name, hy, hx, x, b, tol):
        it = (ctypes.c_int * 2)(); ci = (ctypes.c_int * 2)(); rr = ctypes.c_double(0)
        stores = [h._h if h is not None else None for h in (hy, hx)]
        _check(getattr(self._lib, "ddamg_hip_" + name)(self._h, *stores, x, b, float(tol), it, ci, ctypes.byref(rr)))
        return (it[0], it[1]), (ci[0], ci[1]), rr.value

    def solve_squared_chrono_vec(self, hy, hx, x, b, tol=0.0):
        """D^dagger D x = b, the D^dagger solve from the store hy, the D solve from hx (either may be None: a zero guess); returns as
        solve_squared_vec"""
        return self._squared_chrono_call("solve_squared_chrono_vec", hy, hx, x._h, b._h, tol)

    def solve_squared_chrono_device(self, hy, hx, x_dev_lex, b_dev_lex, tol=0.0):
        n = self.volume(0) * 24
        return self._squared_chrono_call("solve_squared_chrono_device", hy, hx, _dev(x_dev_lex, n, "solve_squared_chrono_device"),
                                         _dev(b_dev_lex, n, "solve_squared_chrono_device"), tol)

    # ---- the even-odd preconditioned system: Dhat = D_ee - D_eo D_oo^-1 D_oe on the even sites (include/ddamg_hip.h) ----
    def vec_upload_parity_device(self, v, parity, half_dev, zero_other=True):
        return v.upload_parity_device(parity, half_dev, zero_other)

    def vec_download_parity_device(self, v, parity, half_dev):
        return v.download_parity_device(parity, half_dev)

    def schur_apply(self, out, inp, dagger=False):
        """out = Dhat inp (dagger: Dhat^dagger inp) on the even sites, zero on the odd ones; the odd sites of inp are not read"""
        _check(self._lib.ddamg_hip_schur_apply(self._h, out._h, inp._h, int(bool(dagger))))

    def schur_apply_device(self, out_e_dev, in_e_dev, dagger=False):
        """the same on half fields of the even sites in device memory; returns out_e_dev"""
        n = self.volume(0) * 12
        _check(self._lib.ddamg_hip_schur_apply_device(self._h, _dev(out_e_dev, n, "schur_apply_device"), _dev(in_e_dev, n, "schur_apply_device"),
                                                      int(bool(dagger))))
        return out_e_dev

    def _schur_call(self, name, head, args, tol, squared=False):
        it = (ctypes.c_int * 2)(); ci = (ctypes.c_int * 2)(); rr = ctypes.c_double(0)
        _check(getattr(self._lib, "ddamg_hip_" + name)(self._h, *head, *args, float(tol), it, ci, ctypes.byref(rr)))
        if squared:
            return (it[0], it[1]), (ci[0], ci[1]), rr.value
        return it[0], ci[0], rr.value

    def _halves(self, name, x_e_dev, x_o_dev, b_e_dev):
        n = self.volume(0) * 12
        return (_dev(x_e_dev, n, name), _dev(x_o_dev, n, name) if x_o_dev is not None else None, _dev(b_e_dev, n, name))

    def solve_schur_vec(self, x, b, tol=0.0, dagger=False, use_guess=False):
        """Dhat x_e = b_e (dagger: Dhat^dagger x_e = b_e) on the even sites of fine fp64 Vectors; use_guess: x holds the guess.  On
        return the odd sites of x hold the odd part of the full-lattice solution.  Returns (iterations, coarse_iterations, relres),
        relres that of the Schur system"""
        return self._schur_call("solve_schur_vec", (int(bool(dagger)), int(bool(use_guess))), (x._h, b._h), tol)

    def solve_schur_device(self, x_e_dev, x_o_dev, b_e_dev, tol=0.0, dagger=False, use_guess=False):
        """the same on half fields in device memory; x_o_dev (may be None) takes the odd part"""
        return self._schur_call("solve_schur_device", (int(bool(dagger)), int(bool(use_guess))),
                                self._halves("solve_schur_device", x_e_dev, x_o_dev, b_e_dev), tol)

    def solve_schur_squared_vec(self, x, b, tol=0.0):
        """Dhat^dagger Dhat x_e = b_e; returns the two pairs of counts and ||b_e - Dhat^dagger Dhat x_e|| / ||b_e|| as solve_squared_vec does"""
        return self._schur_call("solve_schur_squared_vec", (), (x._h, b._h), tol, squared=True)

    def solve_schur_squared_device(self, x_e_dev, x_o_dev, b_e_dev, tol=0.0):
        return self._schur_call("solve_schur_squared_device", (), self._halves("solve_schur_squared_device", x_e_dev, x_o_dev, b_e_dev), tol, squared=True)

    def _multishift_call(self, name, shifts, tols, args, max_iterations):
        n = len(shifts)
        sh = (ctypes.c_double * max(n, 1))(*[float(s) for s in shifts])
        if tols is not None and len(tols) != n:
            raise DDAMGError(f"{name}: {len(tols)} tolerances for {n} shifts")
        tl = (ctypes.c_double * max(n, 1))(*[float(t) for t in tols]) if tols is not None else None
        it = (ctypes.c_int * max(n, 1))(); rr = (ctypes.c_double * max(n, 1))(); rz = (ctypes.c_double * 2)()
        _check(getattr(self._lib, "ddamg_hip_" + name)(self._h, n, sh, tl, *args, int(max_iterations), it, rr, rz))
        return list(it[:n]), list(rr[:n]), (rz[0], rz[1])

    def solve_schur_multishift_vec(self, shifts, xs, b, tols=None, max_iterations=0):
        """x_s = (Dhat^dagger Dhat + shifts[s])^-1 b_e for every shift from one Krylov space (multi-shift CG), on fine fp64 Vectors xs[s]:
        x_s on their even sites, its odd part on the odd ones.  tols: None (params.tol) or one per shift.  Returns (iterations per
        shift, relres per shift, (smallest, largest Ritz value of Dhat^dagger Dhat))"""
        if len(xs) != len(shifts):
            raise DDAMGError(f"solve_schur_multishift_vec: {len(xs)} vectors for {len(shifts)} shifts")
        hs = (ctypes.c_void_p * max(len(xs), 1))(*[x._h for x in xs])
        return self._multishift_call("solve_schur_multishift_vec", shifts, tols, (hs, b._h), max_iterations)

    def solve_schur_multishift_device(self, shifts, x_e_devs, x_o_devs, b_e_dev, tols=None, max_iterations=0):
        """the same on half fields in device memory; x_o_devs: None, or one entry per shift of which any may be None"""
        name = "solve_schur_multishift_device"
        n = self.volume(0) * 12
        if len(x_e_devs) != len(shifts) or (x_o_devs is not None and len(x_o_devs) != len(shifts)):
            raise DDAMGError(f"{name}: one array per shift expected")
        dpp = ctypes.POINTER(ctypes.c_double)
        xe = (dpp * max(len(shifts), 1))(*[_dev(a, n, name) for a in x_e_devs])
        xo = None
        if x_o_devs is not None:
            xo = (dpp * max(len(shifts), 1))(*[_dev(a, n, name) if a is not None else dpp() for a in x_o_devs])
        return self._multishift_call(name, shifts, tols, (xe, xo, _dev(b_e_dev, n, name)), max_iterations)

    def schur_odd_part_device(self, x_o_dev, x_e_dev, dagger=False):
        """x_o_dev = -D_oo^-1 D_oe x_e (dagger: -gamma5 D_oo^-1 D_oe gamma5 x_e) of the even half field x_e_dev; returns x_o_dev"""
        n = self.volume(0) * 12
        _check(self._lib.ddamg_hip_schur_odd_part_device(self._h, int(bool(dagger)), _dev(x_o_dev, n, "schur_odd_part_device"),
                                                         _dev(x_e_dev, n, "schur_odd_part_device")))
        return x_o_dev

    def multishift_update_time(self, nshift, nactive, reps=20):
        """milliseconds per launch of the multi-shift update kernel with the base system and `nactive` further shifts active"""
        ms = ctypes.c_float(0)
        _check(self._lib.ddamg_hip_multishift_update_time(self._h, int(nshift), int(nactive), int(reps), ctypes.byref(ms)))
        return ms.value

    def clover_logdet(self, parity):
        """(sum over the sites of `parity` of log|det D_ss|, sign of the product) of the operator as it is now; collective on a grid"""
        ld = ctypes.c_double(0); sg = ctypes.c_int(0)
        _check(self._lib.ddamg_hip_clover_logdet(self._h, int(parity), ctypes.byref(ld), ctypes.byref(sg)))
        return ld.value, sg.value

    # ---- forces: the derivative of the operator that is set with respect to its links (include/ddamg_hip.h, "Forces") ----
    def force_bilinear_vec(self, force_dev, y, x, coeff=1.0, accumulate=False):
        """force_dev (+)= coeff * the force of Re <y, D x> for fine fp64 Vectors; force_dev: [V][4][9] complex float64 in device
        memory, the layout of the links.  Returns force_dev"""
        _check(self._lib.ddamg_hip_force_bilinear_vec(self._h, _dev(force_dev, self.volume(0) * 72, "force_bilinear_vec"), y._h, x._h, float(coeff),
                                                      int(bool(accumulate))))
        return force_dev

    def force_bilinear_device(self, force_dev, y_dev, x_dev, coeff=1.0, accumulate=False):
        """the same for lexicographic [V][12] complex float64 arrays in device memory; the same bits"""
        V = self.volume(0)
        _check(self._lib.ddamg_hip_force_bilinear_device(self._h, _dev(force_dev, V * 72, "force_bilinear_device"), _dev(y_dev, V * 24, "force_bilinear_device"),
                                                         _dev(x_dev, V * 24, "force_bilinear_device"), float(coeff), int(bool(accumulate))))
        return force_dev

    def force_logdet(self, force_dev, parity, coeff=1.0, accumulate=False):
        """force_dev (+)= coeff * the force of the sum over the sites of `parity` of log|det D_ss| (clover_logdet)"""
        _check(self._lib.ddamg_hip_force_logdet(self._h, _dev(force_dev, self.volume(0) * 72, "force_logdet"), int(parity), float(coeff),
                                                int(bool(accumulate))))
        return force_dev

    def force_bilinear_vec_grid(self, force_dev, y, x, coeff=1.0, accumulate=False):
        """force_bilinear_vec on any process grid: this process's part of the force, the neighbours' shell of the links and of the site
        tensor and their face of x and y exchanged device to device.  Collective: every process of the grid calls it, with a
        transport installed.  On an undivided context it is force_bilinear_vec"""
        _check(self._lib.ddamg_hip_force_bilinear_vec_grid(self._h, _dev(force_dev, self.volume(0) * 72, "force_bilinear_vec_grid"), y._h, x._h,
                                                           float(coeff), int(bool(accumulate))))
        return force_dev

    def force_bilinear_device_grid(self, force_dev, y_dev, x_dev, coeff=1.0, accumulate=False):
        """the same for this process's lexicographic [V_local][12] complex float64 arrays in device memory; the same bits"""
        V = self.volume(0)
        name = "force_bilinear_device_grid"
        _check(self._lib.ddamg_hip_force_bilinear_device_grid(self._h, _dev(force_dev, V * 72, name), _dev(y_dev, V * 24, name), _dev(x_dev, V * 24, name),
                                                              float(coeff), int(bool(accumulate))))
        return force_dev

    def force_logdet_grid(self, force_dev, parity, coeff=1.0, accumulate=False):
        """force_logdet on any process grid (collective); `parity` is the global parity"""
        _check(self._lib.ddamg_hip_force_logdet_grid(self._h, _dev(force_dev, self.volume(0) * 72, "force_logdet_grid"), int(parity), float(coeff),
                                                     int(bool(accumulate))))
        return force_dev

    # ---- the gauge sector of the molecular dynamics (include/ddamg_hip.h, "Gauge sector"): fields are [V][4][9] complex float64 in
    # device memory, links without the anti-periodic sign; not on a process grid ----
    def gauge_loops_device(self, links_dev, rectangles=True):
        """(sum_x sum_{mu<nu} Re tr P, sum_x sum_{mu!=nu} Re tr R) of the links; rectangles=False: the rectangles are not computed
        and None stands in their place.  S = beta [c0 (6 V - plaquettes / 3) + c1 (12 V - rectangles / 3)], c0 = 1 - 8 c1"""
        plaq, rect = ctypes.c_double(0), ctypes.c_double(0)
        _check(self._lib.ddamg_hip_gauge_loops_device(self._h, _dev(links_dev, self.volume(0) * 72, "gauge_loops_device"), ctypes.byref(plaq),
                                                      ctypes.byref(rect) if rectangles else None))
        return plaq.value, (rect.value if rectangles else None)

    def gauge_force_device(self, force_dev, links_dev, beta, c1=0.0, coeff=1.0, accumulate=False):
        """force_dev (+)= coeff * the force of the gauge action (beta, c1: 0 Wilson, -1/12 Symanzik, -0.331 Iwasaki).  Returns force_dev"""
        n = self.volume(0) * 72
        _check(self._lib.ddamg_hip_gauge_force_device(self._h, _dev(force_dev, n, "gauge_force_device"), _dev(links_dev, n, "gauge_force_device"),
                                                      float(beta), float(c1), float(coeff), int(bool(accumulate))))
        return force_dev

    def links_update_device(self, links_dev, mom_dev, eps):
        """U <- exp(eps P) U in place.  Returns links_dev"""
        n = self.volume(0) * 72
        _check(self._lib.ddamg_hip_links_update_device(self._h, _dev(links_dev, n, "links_update_device"), _dev(mom_dev, n, "links_update_device"),
                                                       float(eps)))
        return links_dev

    def links_reunitarize_device(self, links_dev):
        """every link projected back to SU(3) in place (Gram-Schmidt on the first two rows, the third their conjugated cross product).
        Returns the largest |U U^dagger - 1| before the projection"""
        dev = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_links_reunitarize_device(self._h, _dev(links_dev, self.volume(0) * 72, "links_reunitarize_device"), ctypes.byref(dev)))
        return dev.value

    def momentum_update_device(self, mom_dev, force_dev, eps):
        """P <- P + eps F.  Returns mom_dev"""
        n = self.volume(0) * 72
        _check(self._lib.ddamg_hip_momentum_update_device(self._h, _dev(mom_dev, n, "momentum_update_device"), _dev(force_dev, n, "momentum_update_device"),
                                                          float(eps)))
        return mom_dev

    def momentum_kinetic_device(self, mom_dev):
        """1/2 sum |P_ij|^2"""
        kin = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_momentum_kinetic_device(self._h, _dev(mom_dev, self.volume(0) * 72, "momentum_kinetic_device"), ctypes.byref(kin)))
        return kin.value

    # ---- the same six on any process grid: fields are the process's own part, [V_local][4][9].  gauge_loops, gauge_force,
    # momentum_kinetic and (where the deviation is asked for) links_reunitarize are collective; the other two send nothing ----
    def gauge_loops_device_grid(self, links_dev, rectangles=True):
        """gauge_loops_device on any process grid (collective): the sums over the whole lattice, on every process.  The shell of
        the links is two sites deep with rectangles, else one"""
        plaq, rect = ctypes.c_double(0), ctypes.c_double(0)
        _check(self._lib.ddamg_hip_gauge_loops_device_grid(self._h, _dev(links_dev, self.volume(0) * 72, "gauge_loops_device_grid"), ctypes.byref(plaq),
                                                           ctypes.byref(rect) if rectangles else None))
        return plaq.value, (rect.value if rectangles else None)

    def gauge_force_device_grid(self, force_dev, links_dev, beta, c1=0.0, coeff=1.0, accumulate=False):
        """gauge_force_device on any process grid (collective); the bits of the undivided lattice's force.  Returns force_dev"""
        n = self.volume(0) * 72
        _check(self._lib.ddamg_hip_gauge_force_device_grid(self._h, _dev(force_dev, n, "gauge_force_device_grid"),
                                                           _dev(links_dev, n, "gauge_force_device_grid"), float(beta), float(c1), float(coeff),
                                                           int(bool(accumulate))))
        return force_dev

    def links_update_device_grid(self, links_dev, mom_dev, eps):
        """links_update_device on any process grid; nothing is sent.  Returns links_dev"""
        n = self.volume(0) * 72
        _check(self._lib.ddamg_hip_links_update_device_grid(self._h, _dev(links_dev, n, "links_update_device_grid"),
                                                            _dev(mom_dev, n, "links_update_device_grid"), float(eps)))
        return links_dev

    def links_reunitarize_device_grid(self, links_dev, deviation=True):
        """links_reunitarize_device on any process grid.  deviation=True (collective; every process must pass it alike): returns the
        largest |U U^dagger - 1| of the whole lattice before the projection; False: nothing is sent and None is returned"""
        dev = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_links_reunitarize_device_grid(self._h, _dev(links_dev, self.volume(0) * 72, "links_reunitarize_device_grid"),
                                                                 ctypes.byref(dev) if deviation else None))
        return dev.value if deviation else None

    def momentum_update_device_grid(self, mom_dev, force_dev, eps):
        """momentum_update_device on any process grid; nothing is sent.  Returns mom_dev"""
        n = self.volume(0) * 72
        _check(self._lib.ddamg_hip_momentum_update_device_grid(self._h, _dev(mom_dev, n, "momentum_update_device_grid"),
                                                               _dev(force_dev, n, "momentum_update_device_grid"), float(eps)))
        return mom_dev

    def momentum_kinetic_device_grid(self, mom_dev):
        """momentum_kinetic_device on any process grid (collective): 1/2 sum |P_ij|^2 over the whole lattice, on every process"""
        kin = ctypes.c_double(0)
        _check(self._lib.ddamg_hip_momentum_kinetic_device_grid(self._h, _dev(mom_dev, self.volume(0) * 72, "momentum_kinetic_device_grid"),
                                                                ctypes.byref(kin)))
        return kin.value

    def _force_multi_call(self, name, force_dev, ys, xs, weights, coeff, accumulate, convert, ptr):
        n = len(weights)
        if len(ys) != n or len(xs) != n:
            raise DDAMGError(f"{name}: {len(ys)} y, {len(xs)} x for {n} weights: one of each per pair expected")
        ya = (ptr * max(n, 1))(*[convert(a) for a in ys]); xa = (ptr * max(n, 1))(*[convert(a) for a in xs])
        w = (ctypes.c_double * max(n, 1))(*[float(v) for v in weights])
        _check(getattr(self._lib, "ddamg_hip_" + name)(self._h, _dev(force_dev, self.volume(0) * 72, name), n, ya, xa, w, float(coeff),
                                                       int(bool(accumulate))))
        return force_dev

    def force_bilinear_multi_vec(self, force_dev, ys, xs, weights, coeff=1.0, accumulate=False, _name="force_bilinear_multi_vec"):
        """force_dev (+)= coeff * sum_s weights[s] * the force of Re <ys[s], D xs[s]> for lists of fine fp64 Vectors, in one pass: the
        links, the clover derivative and the assembly once, the pairs in groups of FORCE_GROUP.  A vector may repeat.  Returns force_dev"""
        return self._force_multi_call(_name, force_dev, ys, xs, weights, coeff, accumulate, lambda v: v._h if v is not None else None,
                                      ctypes.c_void_p)

    def force_bilinear_multi_device(self, force_dev, y_devs, x_devs, weights, coeff=1.0, accumulate=False, _name="force_bilinear_multi_device"):
        """the same for lists of lexicographic [V][12] complex float64 arrays in device memory; the same bits"""
        n = self.volume(0) * 24
        dpp = ctypes.POINTER(ctypes.c_double)
        return self._force_multi_call(_name, force_dev, y_devs, x_devs, weights, coeff, accumulate, lambda a: _dev(a, n, _name) if a is not None else dpp(), dpp)

    def force_bilinear_multi_vec_grid(self, force_dev, ys, xs, weights, coeff=1.0, accumulate=False):
        """force_bilinear_multi_vec on any process grid (collective): the face spinors of a whole group travel in one message per
        split direction.  On an undivided context it is force_bilinear_multi_vec"""
        return self.force_bilinear_multi_vec(force_dev, ys, xs, weights, coeff, accumulate, _name="force_bilinear_multi_vec_grid")

    def force_bilinear_multi_device_grid(self, force_dev, y_devs, x_devs, weights, coeff=1.0, accumulate=False):
        return self.force_bilinear_multi_device(force_dev, y_devs, x_devs, weights, coeff, accumulate, _name="force_bilinear_multi_device_grid")

    def force_rational_device(self, force_dev, rho, x_e_devs, x_o_devs=None, coeff=1.0, accumulate=False, _name="force_rational_device"):
        """force_dev (+)= coeff * sum_s rho[s] * force_bilinear(Y_s, X_s) with X_s = (x_s, its odd part), Y_s = (Dhat x_s, its dagger odd
        part), built on the device from the even half fields x_e_devs[s] as solve_schur_multishift_device returns them: coeff = -2 gives
        the force of sum_s rho_s phi^dagger (Dhat^dagger Dhat + sigma_s)^-1 phi.  x_o_devs: None, or one entry per shift of which any may
        be None: the odd part is computed inside where it is not given.  Returns force_dev"""
        ns = len(rho)
        n = self.volume(0) * 12
        if len(x_e_devs) != ns or (x_o_devs is not None and len(x_o_devs) != ns):
            raise DDAMGError(f"{_name}: one array per shift expected")
        dpp = ctypes.POINTER(ctypes.c_double)
        conv = lambda a: _dev(a, n, _name) if a is not None else dpp()
        xe = (dpp * max(ns, 1))(*[conv(a) for a in x_e_devs])
        xo = (dpp * max(ns, 1))(*[conv(a) for a in x_o_devs]) if x_o_devs is not None else None
        r = (ctypes.c_double * max(ns, 1))(*[float(v) for v in rho])
        _check(getattr(self._lib, "ddamg_hip_" + _name)(self._h, _dev(force_dev, self.volume(0) * 72, _name), ns, r, xe, xo, float(coeff),
                                                        int(bool(accumulate))))
        return force_dev

    def force_rational_device_grid(self, force_dev, rho, x_e_devs, x_o_devs=None, coeff=1.0, accumulate=False):
        """force_rational_device on any process grid (collective)"""
        return self.force_rational_device(force_dev, rho, x_e_devs, x_o_devs, coeff, accumulate, _name="force_rational_device_grid")

    def preconditioner(self, in_lex):
        a = np.ascontiguousarray(in_lex, dtype=np.float64)
        out = np.empty((self.volume(0), 12, 2))
        _check(self._lib.ddamg_hip_preconditioner(self._h, _dp(out), _dp(a)))
        return out

    def solve_device(self, x_dev_lex, b_dev_lex, tol=0.0):
        """solve with the right-hand side and the solution in device memory ([V][12] complex float64, lexicographic; integer
        addresses or objects with data_ptr()); returns (iterations, coarse_iterations, true relative residual)"""
        return self._solve_dev("solve_device", x_dev_lex, b_dev_lex, tol)

    def preconditioner_device(self, out_dev_lex, in_dev_lex):
        """one V-cycle from / into arrays in device memory; returns out_dev_lex"""
        n = self.volume(0) * 24
        _check(self._lib.ddamg_hip_preconditioner_device(self._h, _dev(out_dev_lex, n, "preconditioner_device"), _dev(in_dev_lex, n, "preconditioner_device")))
        return out_dev_lex

    def residual_history(self):
        n = ctypes.c_int(0)
        buf = np.empty(4096)
        _check(self._lib.ddamg_hip_residual_history(self._h, _dp(buf), 4096, ctypes.byref(n)))
        return buf[:n.value].copy()

    def site_order(self, level=0):
        out = np.empty(self.volume(level), dtype=np.int32)
        _check(self._lib.ddamg_hip_get_site_order(self._h, level, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    # ---- multi-GPU halo exchange ----
    def comm_stats(self, reset=False):
        """what this process sent since the last reset (dict): halo exchanges by payload, global sums, all-gathers"""
        import json
        return json.loads(self._lib.ddamg_hip_comm_stats(self._h, int(bool(reset))).decode() or "{}")

    def comm_init_rccl(self, unique_id):
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        _check(self._lib.ddamg_hip_comm_init_rccl(self._h, ctypes.cast(buf, ctypes.c_void_p)))

    def comm_init_host(self, exchange, allreduce):
        """exchange(list of (send_peer, recv_peer, tag, send: np.uint8 array, recv: np.uint8 array));
        allreduce(np.float64 array) sums it over all processes in place"""
        def trampoline(_user, n, msgs):
            items = []
            for i in range(n):
                m = msgs[i]
                nb = int(m.bytes)
                snd = np.ctypeslib.as_array(ctypes.cast(m.send, ctypes.POINTER(ctypes.c_uint8)), shape=(nb,))
                rcv = np.ctypeslib.as_array(ctypes.cast(m.recv, ctypes.POINTER(ctypes.c_uint8)), shape=(nb,))
                items.append((m.send_peer, m.recv_peer, m.tag, snd, rcv))
            exchange(items)
        def reduce_trampoline(_user, buf, n):
            allreduce(np.ctypeslib.as_array(buf, shape=(n,)))
        self._exchange_cb = EXCHANGE_FN(trampoline)   # keep the callback objects alive
        self._allreduce_cb = ALLREDUCE_FN(reduce_trampoline)
        _check(self._lib.ddamg_hip_comm_init_host(self._h, self._exchange_cb, self._allreduce_cb, None))

    def timer_begin(self):
        _check(self._lib.ddamg_hip_timer_begin(self._h))

    def timer_end(self):
        ms = ctypes.c_float(0)
        _check(self._lib.ddamg_hip_timer_end(self._h, ctypes.byref(ms)))
        return ms.value

    def sync(self):
        _check(self._lib.ddamg_hip_sync(self._h))

    def close(self):
        if self._h:
            self._lib.ddamg_hip_destroy(self._h)
            self._h = ctypes.c_void_p()


def rccl_unique_id():
    buf = ctypes.create_string_buffer(128)
    _check(load_library().ddamg_hip_rccl_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
    return buf.raw


def halo_plan(local_lattice, process_grid, process_coords, face):
    """host-only: (neighbour rank, local lexicographic indices of the face sites in message order)"""
    lib = load_library()
    I4 = ctypes.c_int * 4
    nb = ctypes.c_int(0); cnt = ctypes.c_int(0)
    L, P, C = I4(*local_lattice), I4(*process_grid), I4(*process_coords)
    _check(lib.ddamg_hip_halo_plan(L, P, C, int(face), ctypes.byref(nb), ctypes.byref(cnt), None))
    sites = np.empty(cnt.value, dtype=np.int32)
    if cnt.value:
        _check(lib.ddamg_hip_halo_plan(L, P, C, int(face), ctypes.byref(nb), ctypes.byref(cnt),
                                       sites.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    return nb.value, sites
