"""CPU tests (-m "not gpu"): ILDG configurations and SciDAC/ETMC spinors in the LIME container (include/ddamg_hip_io.h, csrc/lime.cpp,
host code only), the reference's `format: 1` build (src/lime_io.c).  There is no c-lime here to produce a fixture: the library is
held against tests/lime_format.py, an independent Python writer and reader built from the public format description."""
import ctypes, os, re, subprocess
import numpy as np
import pytest
from conftest import load_golden
from ddalphaamg_amd import api, dist as ddist
import ddalphaamg_amd as dd
import lime_format as lf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(1, 1, 1, 1), (2, 1, 1, 1), (1, 2, 1, 2), (2, 2, 2, 2)]
HEADER = dict(vector_type="solution", m0=-0.5, csw=1.0, clov_plaq=1.6479691, hopp_plaq=1.6479691, clov_conf_name="conf/4x4x4x4b6.0000id3n1",
              hopp_conf_name="conf/4x4x4x4b6.0000id3n1")


def grid_coords(P):
    return [ddist.coords_of(r, list(P)) for r in range(int(np.prod(P)))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel()


@pytest.fixture(scope="module")
def conf4():
    g = load_golden("ref_4x4.npz")
    return [int(x) for x in g["conf_dims"]], np.ascontiguousarray(g["gauge"]), float(g["conf_plaq"][0])


@pytest.fixture(scope="module")
def spinor4():
    return np.ascontiguousarray(load_golden("ref_4x4.npz")["dirac_in"])


# container ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plaq", [None, 0.75])
def test_container_of_a_written_configuration(tmp_path, conf4, plaq):
    """record by record: magic (asserted by the parser), version 1, flags 0xC0, types in order, lengths, zero padding, total size"""
    L, U, conf_plaq = conf4
    plaq = conf_plaq if plaq is None else plaq
    path = tmp_path / "conf.ildg"
    api.write_ildg_conf(path, L, U, plaq)
    recs, end = lf.parse(path)
    assert [r[0] for r in recs] == ["ildg-format", "xlf-info", "ildg-binary-data"]
    assert all(r[1] == 0xC0 and r[2] == 1 for r in recs)
    fmt, xlf, data = recs
    assert [lf.tag(fmt[5].decode(), n) for n in ("precision", "lx", "ly", "lz", "lt")] == [64, L[3], L[2], L[1], L[0]]
    assert float(re.fullmatch(r"plaquette = (\S+)\n", xlf[5].decode()).group(1)) == plaq / 3.0       # enough digits to round-trip
    if plaq == 0.75:
        assert xlf[4] == len("plaquette = 0.25\n") == 17        # a text whose length is no multiple of 8: seven zeros behind it
    assert all(r[6] == b"\0" * (lf.pad8(r[4]) - r[4]) for r in recs[:2])
    assert data[4] == U.size * 8
    assert end == os.path.getsize(path) == sum(144 + lf.pad8(r[4]) for r in recs)
    assert data[3] == 144 * 3 + lf.pad8(fmt[4]) + lf.pad8(xlf[4])
    info = api.lime_info(path)
    assert info == dict(kind="gauge", precision=64, lattice=L, has_plaquette=True, plaquette=plaq / 3.0, data_offset=data[3], data_length=data[4],
                        num_records=3)


def test_padding_behind_an_info_text_of_odd_length_is_skipped(tmp_path, conf4):
    """Python-written file: an xlf-info of 29 bytes and a foreign record of 3 bytes before the data"""
    L, U, _ = conf4
    text = "beta = 6\nplaquette = 0.59375\n"
    assert len(text) % 8 == 5
    lf.write_ildg(tmp_path / "c", L, U, 64, xlf_text=text, extra_first=[("scidac-private-file-xml", b"<a>")])
    got, plaq = api.read_ildg_conf(tmp_path / "c", L)
    assert np.array_equal(bits(got), bits(U)) and plaq == 3 * 0.59375
    assert api.lime_info(tmp_path / "c")["num_records"] == 4


# ILDG read ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("P", GRIDS)
def test_ildg_read_on_a_process_grid(tmp_path, conf4, P, precision):
    L, U, conf_plaq = conf4
    path = tmp_path / "conf.ildg"
    lf.write_ildg(path, L, U, precision, plaquette=conf_plaq / 3.0)
    want = U if precision == 64 else U.astype(np.float32).astype(np.float64)
    info = api.lime_info(path)
    assert info["kind"] == "gauge" and info["precision"] == precision and info["lattice"] == L
    assert info["data_length"] == U.size * precision // 8
    # the first link of the record is the X link of site 0
    first = np.fromfile(path, dtype=">f8" if precision == 64 else ">f4", count=18, offset=info["data_offset"]).astype(np.float64)
    assert np.array_equal(first, want[0, 3].ravel()) and not np.array_equal(first, want[0, 0].ravel())
    for C in grid_coords(P):
        part, plaq = api.read_ildg_conf(path, L, P, C)
        assert np.array_equal(bits(part), bits(ddist.local_part(want, L, list(P), C)))
        assert abs(plaq - conf_plaq) <= 1e-14 * conf_plaq
    lf.write_ildg(tmp_path / "noplaq", L, U, precision)
    assert api.read_ildg_conf(tmp_path / "noplaq", L)[1] is None
    assert api.lime_info(tmp_path / "noplaq")["has_plaquette"] is False


# ILDG write ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("P", GRIDS)
def test_ildg_written_by_a_process_grid(tmp_path, conf4, P, precision):
    L, U, conf_plaq = conf4
    path = tmp_path / "conf.ildg"
    for C in reversed(grid_coords(P)):       # the process at the origin need not be the first
        api.write_ildg_conf(path, L, ddist.local_part(U, L, list(P), C), conf_plaq, P, C, precision)
    want = U if precision == 64 else U.astype(np.float32).astype(np.float64)     # numpy rounds to nearest even
    L2, prec2, U2, plaq2 = lf.read_ildg(path)
    assert (L2, prec2) == (L, precision)
    assert np.array_equal(bits(U2), bits(want))
    assert abs(3 * plaq2 - conf_plaq) <= 1e-14 * conf_plaq and plaq2 == conf_plaq / 3.0
    raw = lf.parse(path, keep=1 << 30)[0][2][5]
    assert raw == lf.ildg_bytes(U, precision)
    whole, plaq = api.read_ildg_conf(path, L)
    assert np.array_equal(bits(whole), bits(want)) and abs(plaq - conf_plaq) <= 1e-14 * conf_plaq


# vectors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", GRIDS)
def test_vector_written_by_a_process_grid(tmp_path, spinor4, P):
    L = [4, 4, 4, 4]; v = spinor4
    path = tmp_path / "vec.lime"
    for C in reversed(grid_coords(P)):
        api.write_lime_vector(path, L, ddist.local_part(v, L, list(P), C), HEADER, P, C)
    recs, end = lf.parse(path, keep=1 << 30)
    assert [r[0] for r in recs] == ["vector-type", "etmc-propagator-format", "dd_alpha_amg-header", "scidac-binary-data"]
    assert all(r[1] == 0xC0 and r[2] == 1 and r[6] == b"\0" * (lf.pad8(r[4]) - r[4]) for r in recs)
    assert end == os.path.getsize(path)
    assert recs[0][5] == b"Vector_by_DDalphaAMG"
    xml = recs[1][5].decode()
    assert "<field>diracFermion</field>" in xml
    assert [lf.tag(xml, n) for n in ("precision", "flavours", "lx", "ly", "lz", "lt", "spin", "colour")] == [64, 1, 4, 4, 4, 4, 4, 3]
    text = recs[2][5].decode().split("\n")
    assert text[0] == "<header>" and text[-1] == "</header>"
    for line in ("\tm0: -0.50000000000000", "\tcsw: 1.00000000000000", "\tclov plaq: 1.64796910000000", "\tclov conf name: conf/4x4x4x4b6.0000id3n1",
                 "\tX: 4", "\tT: 4", "\tX local: %d" % (4 // P[3]), "\tT local: %d" % (4 // P[0])):
        assert line in text, line
    assert np.array_equal(np.frombuffer(recs[3][5], dtype=">f8").astype(np.float64).view(np.uint64), bits(v))
    info = api.lime_info(path)
    assert info["kind"] == "vector" and info["precision"] == 64 and info["lattice"] == L and info["num_records"] == 4
    assert info["data_offset"] == recs[3][3] and info["data_length"] == v.size * 8
    for C in grid_coords(P):
        assert np.array_equal(bits(api.read_lime_vector(path, L, P, C)), bits(ddist.local_part(v, L, list(P), C)))


def test_single_precision_source_file_is_read_exactly(tmp_path, spinor4):
    L = [4, 4, 4, 4]
    lf.write_vector(tmp_path / "src", L, spinor4, 32, "etmc-source-format")
    want = spinor4.astype(np.float32).astype(np.float64)
    assert np.array_equal(bits(api.read_lime_vector(tmp_path / "src", L)), bits(want))
    part = api.read_lime_vector(tmp_path / "src", L, (1, 2, 1, 2), (0, 1, 0, 1))
    assert np.array_equal(bits(part), bits(ddist.local_part(want, L, [1, 2, 1, 2], [0, 1, 0, 1])))
    lf.write_vector(tmp_path / "bare", L, spinor4, 64)
    api.write_lime_vector(tmp_path / "nohdr", L, spinor4)          # header == NULL
    for f in ("bare", "nohdr"):
        assert np.array_equal(bits(api.read_lime_vector(tmp_path / f, L)), bits(spinor4))


# 64-bit offsets -----------------------------------------------------------------------------------------------------------
def test_record_beyond_four_gigabytes(tmp_path):
    """a sparse 32x64x64x64 fp64 configuration: one non-zero link at the last site, behind byte 2^32"""
    L = [32, 64, 64, 64]; V = int(np.prod(L))
    length = V * 72 * 8
    assert length > 2 ** 32
    path = tmp_path / "big.ildg"
    fmt = lf.record("ildg-format", lf.ildg_format_xml(L, 64).encode())
    offset = len(fmt) + 144
    link = np.arange(1, 19, dtype=np.float64) / 16
    try:
        with open(path, "wb") as f:
            f.write(fmt)
            f.write(lf.header("ildg-binary-data", length))
            f.truncate(offset + length)
            f.seek(offset + length - 18 * 8)       # the last 18 doubles of the record: the T link (file order X,Y,Z,T) of the last site
            f.write(link.astype(">f8").tobytes())
        if os.stat(path).st_blocks * 512 > (64 << 20):
            raise OSError("the file is not sparse")
    except OSError as e:
        if os.path.exists(path):
            os.remove(path)
        pytest.skip(f"the filesystem refuses a sparse file of {offset + length} bytes: {e}")
    try:
        info = api.lime_info(path)
        assert info["kind"] == "gauge" and info["data_length"] == length == 4831838208 and info["data_offset"] == offset and info["lattice"] == L
        P = (4, 4, 4, 4)
        part, plaq = api.read_ildg_conf(path, L, P, (3, 3, 3, 3))
        assert plaq is None and part.shape[0] == V // 256
        assert np.array_equal(part[-1, 0].ravel(), link)          # our order T,Z,Y,X: direction 0 of the last local site
        assert np.count_nonzero(part) == 18
        other, _ = api.read_ildg_conf(path, L, P, (3, 3, 3, 2))
        assert np.count_nonzero(other) == 0
    finally:
        os.remove(path)


# refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path, conf4, spinor4):
    L, U, plaq = conf4
    good = tmp_path / "good"
    api.write_ildg_conf(good, L, U, plaq)
    raw = open(good, "rb").read()

    def local_volume(lattice, grid):
        return int(np.prod([g // p for g, p in zip(lattice, grid)]))

    def refused(path, match, lattice=L, grid=(1, 1, 1, 1), coords=(0, 0, 0, 0)):
        out = np.full((local_volume(lattice, grid), 4, 9, 2), 7.5)
        with pytest.raises(api.DDAMGError, match=match):
            api.read_ildg_conf(path, lattice, grid, coords, out=out)
        assert np.all(out == 7.5)           # a failed read leaves the output untouched

    refused(tmp_path / "missing", "cannot open")
    open(tmp_path / "magic", "wb").write(b"\x45\x67\x89\xac" + raw[4:])
    refused(tmp_path / "magic", "not a LIME file")
    open(tmp_path / "plain", "wb").write(np.asarray(L, dtype="<i4").tobytes() + U.tobytes())      # the reference's own format
    refused(tmp_path / "plain", "not a LIME file")
    with open(tmp_path / "nodata", "wb") as f:
        f.write(lf.record("ildg-format", lf.ildg_format_xml(L, 64).encode()))
    refused(tmp_path / "nodata", "no binary record")
    with open(tmp_path / "noformat", "wb") as f:
        f.write(lf.record("ildg-binary-data", lf.ildg_bytes(U, 64)))
    refused(tmp_path / "noformat", "no format record")
    with open(tmp_path / "halfformat", "wb") as f:
        f.write(lf.record("ildg-format", lf.ildg_format_xml(L, 64).replace("<lz>4</lz>", "").encode()))
        f.write(lf.record("ildg-binary-data", lf.ildg_bytes(U, 64)))
    refused(tmp_path / "halfformat", "incomplete format record")
    refused(good, "expected 8x4x4x4", lattice=[8, 4, 4, 4])
    with open(tmp_path / "length", "wb") as f:          # an fp32 record under a format record that says 64
        f.write(lf.record("ildg-format", lf.ildg_format_xml(L, 64).encode()))
        f.write(lf.record("ildg-binary-data", lf.ildg_bytes(U, 32)))
    refused(tmp_path / "length", "binary record has 73728 bytes")
    open(tmp_path / "short", "wb").write(raw[:len(raw) - 1000])
    refused(tmp_path / "short", "ends early")
    open(tmp_path / "header", "wb").write(raw[:100])
    refused(tmp_path / "header", "ends early")
    refused(good, "does not divide", grid=(3, 1, 1, 1))
    refused(good, "does not divide", grid=(2, 1, 1, 1), coords=(2, 0, 0, 0))
    for call in (lambda: api.lime_info(tmp_path / "missing"), lambda: api.lime_info(tmp_path / "magic"), lambda: api.lime_info(tmp_path / "short")):
        with pytest.raises(api.DDAMGError):
            call()
    assert api.lime_info(tmp_path / "nodata")["kind"] is None
    with pytest.raises(api.DDAMGError, match="does not divide"):
        api.write_ildg_conf(tmp_path / "w", L, U, plaq, (3, 1, 1, 1))
    with pytest.raises(api.DDAMGError, match="precision must be 32 or 64"):
        api.write_ildg_conf(tmp_path / "w", L, U, plaq, precision=16)
    with pytest.raises(api.DDAMGError, match="cannot create"):
        api.write_ildg_conf(tmp_path / "nodir" / "w", L, U, plaq)
    # vectors
    vec = tmp_path / "vec"
    api.write_lime_vector(vec, [4] * 4, spinor4, HEADER)
    for path, lattice, grid, match, setup in (
            (tmp_path / "missing", [4] * 4, (1, 1, 1, 1), "cannot open", None),
            (good, [4] * 4, (1, 1, 1, 1), "no binary record", None),                         # a configuration is no vector
            (vec, [4, 4, 4, 8], (1, 1, 1, 1), "expected 4x4x4x8", None),
            (vec, [4] * 4, (1, 3, 1, 1), "does not divide", None),
            (tmp_path / "flavours", [4] * 4, (1, 1, 1, 1), "flavours 2", lambda p: lf.write_vector(p, [4] * 4, np.concatenate([spinor4, spinor4]), flavours=2)),
            (tmp_path / "colour", [4] * 4, (1, 1, 1, 1), "colour 2", lambda p: lf.write_vector(p, [4] * 4, spinor4, colour=2)),
            (tmp_path / "spin", [4] * 4, (1, 1, 1, 1), "spin 2", lambda p: lf.write_vector(p, [4] * 4, spinor4, spin=2)),
            (tmp_path / "veclen", [4] * 4, (1, 1, 1, 1), "binary record has", lambda p: lf.write_vector(p, [4] * 4, spinor4[:200])),
            (tmp_path / "vecshort", [4] * 4, (1, 1, 1, 1), "ends early", lambda p: open(p, "wb").write(open(vec, "rb").read()[:-8]))):
        if setup:
            setup(path)
        out = np.full((local_volume(lattice, grid), 12, 2), 7.5)
        with pytest.raises(api.DDAMGError, match=match):
            api.read_lime_vector(path, lattice, grid, out=out)
        assert np.all(out == 7.5)
    with open(tmp_path / "vecnoformat", "wb") as f:
        f.write(lf.record("scidac-binary-data", spinor4.astype(">f8").tobytes()))
    with pytest.raises(api.DDAMGError, match="no format record"):
        api.read_lime_vector(tmp_path / "vecnoformat", [4] * 4)


# plumbing -----------------------------------------------------------------------------------------------------------------
cs, ip, dp, vp = ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
IO_SYMBOLS = {
    "ddamg_hip_lime_info": ([cs, ctypes.POINTER(api.LimeInfo)], "lime_info"),
    "ddamg_hip_read_ildg_conf": ([cs, ip, ip, ip, dp, dp, ip], "read_ildg_conf"),
    "ddamg_hip_write_ildg_conf": ([cs, ip, ip, ip, ctypes.c_int, dp, ctypes.c_double], "write_ildg_conf"),
    "ddamg_hip_read_lime_vector": ([cs, ip, ip, ip, dp], "read_lime_vector"),
    "ddamg_hip_write_lime_vector": ([cs, ip, ip, ip, ctypes.POINTER(api.VectorHeader), dp], "write_lime_vector"),
}
CTX_SYMBOLS = {
    "ddamg_hip_ildg_to_links_device": ([vp, vp, ctypes.c_int, ctypes.c_longlong, dp], "ildg_to_links_device",
                                       "int ddamg_hip_ildg_to_links_device(ddamg_hip_ctx* ctx, const void* raw_dev, int precision, long long nsites, double* links_dev);"),
    "ddamg_hip_links_to_ildg_device": ([vp, dp, ctypes.c_int, ctypes.c_longlong, vp], "links_to_ildg_device",
                                       "int ddamg_hip_links_to_ildg_device(ddamg_hip_ctx* ctx, const double* links_dev, int precision, long long nsites, void* raw_dev);"),
    "ddamg_hip_load_ildg_conf": ([vp, cs, ctypes.c_int, dp, dp, ip], "load_ildg_conf",
                                 "int ddamg_hip_load_ildg_conf(ddamg_hip_ctx* ctx, const char* path, int anti_pbc, double* plaquette_out, double* file_plaquette_out, int* has_file_plaquette_out);"),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(dd.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return api._io()


@pytest.mark.parametrize("name", sorted(IO_SYMBOLS))
def test_file_entry_point_is_declared_exported_and_mirrored(lib, name):
    types, mirror = IO_SYMBOLS[name]
    assert name in dd.declared_symbols()
    assert re.search(r"\bint %s\(" % name, open(os.path.join(REPO, "include", "ddamg_hip_io.h")).read())
    assert getattr(lib, name).argtypes == types
    assert callable(getattr(api, mirror))


@pytest.mark.parametrize("name", sorted(CTX_SYMBOLS))
def test_device_entry_point_is_declared_exported_and_mirrored(lib, name):
    types, method, declaration = CTX_SYMBOLS[name]
    assert name in dd.declared_symbols()
    assert declaration in re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "ddamg_hip.h")).read())
    entry = getattr(lib, name)
    assert entry.argtypes == types and entry.restype == ctypes.c_int
    assert callable(getattr(api.Context, method))
    # a null context is an error with a message, not a crash
    assert entry(*[None if t in (vp, dp, ip, cs) else t(0) for t in types]) != 0 and lib.ddamg_hip_last_error()


def test_lime_info_struct_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "ddamg_hip_io.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"struct ddamg_hip_lime_info \{(.*?)\};", hdr, flags=re.S).group(1), flags=re.S)
    names = [re.findall(r"([A-Za-z_][A-Za-z_0-9]*)\s*(?:\[[^\]]*\])?\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in api.LimeInfo._fields_]


def test_chunk_knob_is_in_the_table_of_switches():
    """DDAMG_ILDG_CHUNK_SITES: an optional integer of knobs.h, read with the others, documented with the others"""
    knobs = open(os.path.join(REPO, "ddalphaamg_amd", "csrc", "knobs.h")).read()
    assert "OptionalInt ildg_chunk_sites;" in knobs and 'k.ildg_chunk_sites = integer("DDAMG_ILDG_CHUNK_SITES");' in knobs
    assert "DDAMG_ILDG_CHUNK_SITES" in open(os.path.join(REPO, "docs", "design", "07_scope_knobs_pcie.md")).read()


# the host code under sanitizers ----------------------------------------------------------------------------------------------
def test_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """lime.cpp and io.cpp are host code: a stand-alone program (tests/native/lime_roundtrip.cpp, its own main) built by the host
    compiler with -fsanitize=address,undefined, runtimes linked statically, writes and reads the 4^4 cases and walks the refusals"""
    import shutil
    cxx = next((c for c in ("c++", "g++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler with static sanitizer runtimes (c++ / g++)")
    csrc = os.path.join(REPO, "ddalphaamg_amd", "csrc")
    exe = tmp_path / "lime_roundtrip"
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-I", os.path.join(REPO, "include"), "-I", csrc, "-o", str(exe),
                            os.path.join(REPO, "tests", "native", "lime_roundtrip.cpp"), os.path.join(csrc, "lime.cpp"), os.path.join(csrc, "io.cpp")],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("libasan" in build.stderr or "libubsan" in build.stderr):
        pytest.skip("the host compiler has no static sanitizer runtimes: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    work = tmp_path / "files"; work.mkdir()
    run = subprocess.run([str(exe), str(work)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "LIME_ROUNDTRIP_OK" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
