"""ILDG configurations on the device (-m gpu): the conversion kernels of csrc/ildg_device.hip against numpy's decode, and
ddamg_hip_load_ildg_conf (file -> pinned staging -> device links -> operator) against the reference's dumps and against
ddamg_hip_set_gauge of the same links.  Files are written by tests/lime_format.py, the independent Python writer."""
import ctypes, os
import numpy as np
import pytest
from conftest import relerr
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import lime_format as lf
import test_gpu_device_interface as di
from test_gpu_device_interface import Hip, params, check_dirac, synth_field

pytestmark = pytest.mark.gpu
RAGGED = di.RAGGED
SENTINELS = 64


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def upload_bytes(hip, raw):
    p = hip.alloc(max(len(raw), 16))
    buf = np.frombuffer(raw, dtype=np.uint8)
    assert hip.lib.hipMemcpy(p, buf.ctypes.data, buf.nbytes, 1) == 0
    return p


def download_bytes(hip, p, n):
    out = np.empty(n, dtype=np.uint8)
    assert hip.lib.hipMemcpy(out.ctypes.data, p, n, 2) == 0
    return out.tobytes()


def special_links(nsites, precision):
    """links [nsites][4][9][2] whose values are exactly representable in the file's precision, with -0.0, a subnormal, +-inf and a
    quiet NaN with a payload among them"""
    rng = np.random.default_rng(100 + nsites)
    a = rng.standard_normal((nsites, 4, 9, 2))
    if precision == 32:
        a = a.astype(np.float32).astype(np.float64)
        nan = np.array([0x7FC12345], dtype=np.uint32).view(np.float32).astype(np.float64)[0]
        sub = float(np.float32(1e-41))
    else:
        nan = np.array([0x7FF8000012345678], dtype=np.uint64).view(np.float64)[0]
        sub = 5e-320
    flat = a.reshape(-1)
    for k, v in enumerate((-0.0, sub, np.inf, -np.inf, nan, -sub)):
        flat[(7 * k + 3) % flat.size] = v          # within the first site, so that nsites = 1 has them all
    return a


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel()


@pytest.fixture(scope="module")
def ctx4():
    c = dd.Context(params([4] * 4, [2] * 4, -0.5, 1.0))
    yield c
    c.close()


# 1 kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("nsites", [1, 63, 64, 65, 257])
def test_conversion_kernels(ctx4, hip, nsites, precision):
    U = special_links(nsites, precision)
    raw = lf.ildg_bytes(U, precision)               # numpy: direction reversal, rounding, big endian
    assert len(raw) == nsites * 72 * precision // 8
    want = lf.ildg_links(raw, precision)            # numpy's decode
    assert np.array_equal(bits(want), bits(U))
    d_raw = upload_bytes(hip, raw)
    sentinel = np.full(SENTINELS, 123.25)
    d_links = hip.upload(np.concatenate([np.zeros(nsites * 72), sentinel]))
    ctx4.ildg_to_links_device(d_raw, precision, nsites, d_links)
    got = hip.download(d_links, (nsites * 72 + SENTINELS,))
    assert np.array_equal(bits(got[:nsites * 72]), bits(want))
    assert np.array_equal(got[nsites * 72:], sentinel)
    assert download_bytes(hip, d_raw, len(raw)) == raw               # the input is not written
    # the inverse: the raw bytes back (fp64), the rounded ones (fp32) from links that need rounding
    V = U if precision == 64 else special_links(nsites, 64)
    back = lf.ildg_bytes(V, precision)
    d_in = hip.upload(V)
    d_out = upload_bytes(hip, b"\xa5" * (len(back) + SENTINELS))
    ctx4.links_to_ildg_device(d_in, precision, nsites, d_out)
    out = download_bytes(hip, d_out, len(back) + SENTINELS)
    if precision == 64:
        assert out[:len(back)] == back == raw
    else:
        a = np.frombuffer(out[:len(back)], dtype=">u4"); b = np.frombuffer(back, dtype=">u4")
        nan = np.isnan(np.frombuffer(back, dtype=">f4"))
        assert np.array_equal(a[~nan], b[~nan])                          # round to nearest even, as numpy rounds
        assert np.all(np.isnan(np.frombuffer(out[:len(back)], dtype=">f4")[nan]))   # NaN stays NaN; which payload bits survive the narrowing is the hardware's
    assert out[len(back):] == b"\xa5" * SENTINELS
    assert np.array_equal(bits(hip.download(d_in, V.shape)), bits(V))


def test_conversion_refusals(ctx4, hip):
    n = 8
    d_raw = upload_bytes(hip, bytes(n * 72 * 8)); d_links = hip.upload(np.zeros(n * 72))
    host = np.zeros(n * 72)
    for raw, links, match in ((0, d_links, "null pointer"), (d_raw, 0, "null pointer"), (int(host.ctypes.data), d_links, "not a pointer into device memory"),
                              (d_raw, int(host.ctypes.data), "not a pointer into device memory"), (d_links, d_links, "overlap"),
                              (d_links + 16, d_links, "smaller than the array"), (d_raw + 8, d_links, "aligned")):
        nsites = n - 1 if match == "aligned" else n
        for call in (lambda: ctx4.ildg_to_links_device(raw, 64, nsites, links), lambda: ctx4.links_to_ildg_device(links, 64, nsites, raw)):
            with pytest.raises(api.DDAMGError, match=match):
                call()
    big = hip.upload(np.zeros(2 * n * 72))
    with pytest.raises(api.DDAMGError, match="overlap"):             # the fp32 record inside the link array
        ctx4.ildg_to_links_device(big + n * 72 * 4, 32, n, big)
    with pytest.raises(api.DDAMGError, match="precision must be 32 or 64"):
        ctx4.ildg_to_links_device(d_raw, 16, n, d_links)
    assert np.array_equal(hip.download(d_links, (n * 72,)), np.zeros(n * 72))


# 2 the reference's 4^4 dumps ----------------------------------------------------------------------------------------------
def test_load_of_the_golden_configuration_in_three_chunks(gold4, tmp_path, monkeypatch):
    """bounds of test_reference_dumps_4 (test_gpu_device_interface.py): the same downstream kernels"""
    path = tmp_path / "conf.ildg"
    lf.write_ildg(path, [4] * 4, gold4["gauge"], 64, plaquette=float(gold4["conf_plaq"][0]) / 3.0)
    monkeypatch.setenv("DDAMG_ILDG_CHUNK_SITES", "96")       # 96 + 96 + a 64-site tail
    ctx = dd.Context(params([4] * 4, [2] * 4, float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])))
    plaq, file_plaq = ctx.load_ildg_conf(path, anti_pbc=True)
    print("plaquette", plaq, "file", file_plaq, "dump", float(gold4["meta_f64"][2]))
    assert abs(plaq - float(gold4["meta_f64"][2])) < 1e-12
    assert abs(file_plaq - float(gold4["conf_plaq"][0])) <= 1e-14 * float(gold4["conf_plaq"][0])
    D, cl = ctx.get_operator()
    print("clover relerr", relerr(cl, gold4["clover"]))
    assert np.array_equal(D, gold4["D"])
    assert relerr(cl, gold4["clover"]) < 1e-14
    check_dirac(ctx, gold4)
    ctx.close()


# 3 a lattice no tile divides ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    """the field, and per (precision, anti_pbc) what set_gauge makes of it (computed once)"""
    U = synth_field(RAGGED, 7)
    fields = {64: U, 32: U.astype(np.float32).astype(np.float64)}
    ref = {}
    for precision, F in fields.items():
        for anti_pbc in (0, 1):
            host = dd.Context(params(RAGGED, [2] * 4, -0.3, 1.25))
            plaq = host.set_gauge(F, anti_pbc=bool(anti_pbc))
            ref[precision, anti_pbc] = (plaq,) + host.get_operator()
            host.close()
    return U, ref


@pytest.mark.parametrize("chunk", [500, None])
@pytest.mark.parametrize("anti_pbc", [0, 1])
@pytest.mark.parametrize("precision", [64, 32])
def test_load_on_a_lattice_no_tile_divides(ragged, tmp_path, monkeypatch, precision, anti_pbc, chunk):
    U, ref = ragged
    path = tmp_path / "conf.ildg"
    lf.write_ildg(path, RAGGED, U, precision)
    if chunk:
        monkeypatch.setenv("DDAMG_ILDG_CHUNK_SITES", str(chunk))      # 1920 sites: 500 x 3 + a 420-site tail
    else:
        monkeypatch.delenv("DDAMG_ILDG_CHUNK_SITES", raising=False)
    ctx = dd.Context(params(RAGGED, [2] * 4, -0.3, 1.25))
    plaq, file_plaq = ctx.load_ildg_conf(path, anti_pbc=bool(anti_pbc))
    D, cl = ctx.get_operator()
    ctx.close()
    plaq_h, Dh, clh = ref[precision, anti_pbc]
    print("clover relerr", relerr(cl, clh), "plaquette", plaq, plaq_h)
    assert file_plaq is None
    assert np.array_equal(D, Dh)
    assert relerr(cl, clh) < 1e-14
    assert abs(plaq - plaq_h) < 1e-12


# 4 process grid -----------------------------------------------------------------------------------------------------------
def test_load_on_the_self_exchange_grid(gold4, hip, tmp_path):
    m0, csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    path = tmp_path / "conf.ildg"
    lf.write_ildg(path, [4] * 4, gold4["gauge"], 64, plaquette=float(gold4["conf_plaq"][0]) / 3.0)
    grid = dd.Context(params([4] * 4, [2] * 4, m0, csw, grid=(-1, 1, 1, 1)))
    grid.comm_init_rccl(api.rccl_unique_id())
    plaq_h = grid.set_gauge(gold4["gauge"], anti_pbc=True)
    Dh, clh = grid.get_operator()
    grid.set_gauge(np.ascontiguousarray(gold4["gauge"][::-1]), anti_pbc=True)        # another operator in between
    plaq, file_plaq = grid.load_ildg_conf(path, anti_pbc=True)
    D, cl = grid.get_operator()
    assert np.array_equal(D, Dh) and relerr(cl, clh) < 1e-14 and abs(plaq - plaq_h) < 1e-12
    assert abs(file_plaq - float(gold4["conf_plaq"][0])) <= 1e-14 * float(gold4["conf_plaq"][0])
    check_dirac(grid, gold4)
    with pytest.raises(api.DDAMGError, match="ddamg_hip_set_gauge"):
        grid.set_gauge_device(hip.upload(gold4["gauge"]), anti_pbc=True)
    check_dirac(grid, gold4)
    grid.close()


# 5 memory and failures ----------------------------------------------------------------------------------------------------
def test_memory_and_failed_loads(gold4, hip, tmp_path, monkeypatch):
    m0, csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    path = tmp_path / "conf.ildg"
    lf.write_ildg(path, [4] * 4, gold4["gauge"], 64)
    monkeypatch.setenv("DDAMG_ILDG_CHUNK_SITES", "100")
    before = api.memory_in_use()
    dev = dd.Context(params([4] * 4, [2] * 4, m0, csw))
    dev.set_gauge_device(hip.upload(gold4["gauge"]), anti_pbc=True)
    with_device = api.memory_in_use()
    dev.close()
    assert api.memory_in_use() == before
    ctx = dd.Context(params([4] * 4, [2] * 4, m0, csw))
    ctx.load_ildg_conf(path, anti_pbc=True)
    assert api.memory_in_use() == with_device          # the link array, the raw chunk and the pinned staging are released
    check_dirac(ctx, gold4)
    with_vectors = api.memory_in_use()                 # the context's staging buffer for vector uploads stays
    lf.write_ildg(tmp_path / "other", [4, 4, 4, 8], np.zeros((512, 4, 9, 2)), 64)
    open(tmp_path / "short", "wb").write(open(path, "rb").read()[:-4096])
    for bad, match in ((tmp_path / "other", "expected 4x4x4x4"), (tmp_path / "missing", "cannot open"), (tmp_path / "short", "ends early")):
        with pytest.raises(api.DDAMGError, match=match):
            ctx.load_ildg_conf(bad, anti_pbc=True)
        assert api.memory_in_use() == with_vectors
        check_dirac(ctx, gold4)                        # the operator set before is in place
    ctx.close()
    assert api.memory_in_use() == before
