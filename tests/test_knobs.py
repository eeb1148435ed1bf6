"""CPU tests of ddalphaamg_amd/csrc/knobs.h, the one place where the library reads its DDAMG_* environment switches: a host
program that includes nothing but that header prints every field of Knobs::from_env() under a handful of environments, and
the parse rules (they are not uniform) are compared with the table below.  No GPU, no library load."""
import os, shutil, subprocess
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ddalphaamg_amd", "csrc")

# on for ANY value, "0" included
PRESENCE = {
    "DDAMG_GALERKIN_UNBATCHED": "galerkin_unbatched", "DDAMG_GALERKIN_FULL_FIELDS": "galerkin_full_fields",
    "DDAMG_GALERKIN_STORE_COLUMNS": "galerkin_store_columns", "DDAMG_BOOTSTRAP_UNBATCHED": "bootstrap_unbatched",
    "DDAMG_TV_GS_COLUMNWISE": "tv_gs_columnwise", "DDAMG_GS_WORKGROUP": "gs_workgroup", "DDAMG_COARSE_GS_GLOBAL": "coarse_gs_global",
    "DDAMG_AGGREGATE_DIRAC_GATHER": "aggregate_dirac_gather", "DDAMG_COARSE_RESTRICT_VALU": "coarse_restrict_valu",
    "DDAMG_COARSE_SAP_UNFUSED": "coarse_sap_unfused", "DDAMG_PIPELINED_ARNOLDI": "pipelined_arnoldi",
    "DDAMG_SINGLE_ALLREDUCE_ARNOLDI": "single_allreduce_arnoldi", "DDAMG_SETUP_TIMING": "setup_timing", "DDAMG_POISON": "poison",
}
DEFAULTS = dict({f: 0 for f in PRESENCE.values()},
                link_compression=1, clover_compression=1, sap_variant=3, coarse_gs_workgroup_form=0,
                coarse_apply_once_min_sites=2048, host_transport=0,
                galerkin_slab_aggs_set=0, galerkin_slab_aggs=0, bootstrap_group_set=0, bootstrap_group=0, comm_cus_set=0, comm_cus=0,
                comm_cus_1_level=24, comm_cus_3_levels=0)

PROBE = r"""
#include "knobs.h"
#include <cstdio>
int main() {
  const ddamg::Knobs k = ddamg::Knobs::from_env();
#define F(name) printf(#name "=%d\n", (int)k.name);
#define O(name) printf(#name "_set=%d\n" #name "=%d\n", (int)k.name.set, k.name.value);
  F(link_compression) F(clover_compression) F(sap_variant) F(galerkin_unbatched) F(galerkin_full_fields) F(galerkin_store_columns)
  O(galerkin_slab_aggs) F(aggregate_dirac_gather) F(coarse_restrict_valu) F(bootstrap_unbatched) O(bootstrap_group) F(tv_gs_columnwise)
  F(gs_workgroup) F(coarse_gs_global) F(coarse_gs_workgroup_form) F(coarse_sap_unfused) F(coarse_apply_once_min_sites)
  F(pipelined_arnoldi) F(single_allreduce_arnoldi) O(comm_cus) F(host_transport) F(setup_timing)
  printf("comm_cus_1_level=%d\ncomm_cus_3_levels=%d\npoison=%d\n", ddamg::comm_cus_for(k, 1), ddamg::comm_cus_for(k, 3), (int)ddamg::poison_allocations());
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """the probe program, built by the host C++ compiler (hipcc in host-only mode where there is no other)"""
    d = tmp_path_factory.mktemp("knobs")
    src = d / "probe.cpp"; exe = d / "probe"
    src.write_text(PROBE)
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [cxx] if cxx else [hipcc, "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)

    def run(**env):
        out = subprocess.run([str(exe)], env={"DDAMG_" + k: v for k, v in env.items()}, check=True, capture_output=True, text=True).stdout
        return {k: int(v) for k, v in (line.split("=") for line in out.split())}
    return run


def expect(**changed):
    return dict(DEFAULTS, **changed)


def test_defaults_with_an_empty_environment(probe):
    got = probe()
    assert got == DEFAULTS
    assert set(got) == set(DEFAULTS)       # the probe prints every field of the table, and nothing else


def test_presence_switches_are_on_for_any_value(probe):
    got = probe(**{name[len("DDAMG_"):]: "0" for name in PRESENCE})
    assert got == expect(**{f: 1 for f in PRESENCE.values()})
    for name, field in PRESENCE.items():   # ... and each of them moves its own field only
        assert probe(**{name[len("DDAMG_"):]: ""}) == expect(**{field: 1}), name


@pytest.mark.parametrize("switch,field", [("LINK_COMPRESSION", "link_compression"), ("CLOVER_COMPRESSION", "clover_compression")])
def test_compression_switches_are_off_only_when_set_to_zero(probe, switch, field):
    assert probe(**{switch: "0"}) == expect(**{field: 0})
    assert probe(**{switch: "1"}) == DEFAULTS
    assert probe(**{switch: "off"}) == expect(**{field: 0})    # atoi("off") == 0, as before


def test_coarse_gs_form_is_tested_by_its_first_character(probe):
    assert probe(COARSE_GS_FORM="workgroup") == expect(coarse_gs_workgroup_form=1)
    assert probe(COARSE_GS_FORM="w") == expect(coarse_gs_workgroup_form=1)
    assert probe(COARSE_GS_FORM="x") == DEFAULTS
    assert probe(COARSE_GS_FORM="") == DEFAULTS


def test_integer_switches(probe):
    assert probe(SAP_VARIANT="1") == expect(sap_variant=1)
    assert probe(COARSE_APPLY_ONCE_MIN_SITES="0") == expect(coarse_apply_once_min_sites=0)
    # the clamps are applied where these two are used: "set" has to stay distinguishable from every value
    assert probe(GALERKIN_SLAB_AGGS="5") == expect(galerkin_slab_aggs_set=1, galerkin_slab_aggs=5)
    assert probe(GALERKIN_SLAB_AGGS="0") == expect(galerkin_slab_aggs_set=1, galerkin_slab_aggs=0)
    assert probe(BOOTSTRAP_GROUP="5") == expect(bootstrap_group_set=1, bootstrap_group=5)


def test_comm_cus_by_level_count_unless_set(probe):
    assert probe() == expect(comm_cus_1_level=24, comm_cus_3_levels=0)
    assert probe(COMM_CUS="0") == expect(comm_cus_set=1, comm_cus=0, comm_cus_1_level=0, comm_cus_3_levels=0)
    assert probe(COMM_CUS="16") == expect(comm_cus_set=1, comm_cus=16, comm_cus_1_level=16, comm_cus_3_levels=16)


def test_transport(probe):
    assert probe(HIP_TRANSPORT="host") == expect(host_transport=1)
    assert probe(HIP_TRANSPORT="rccl") == DEFAULTS
    assert probe(HIP_TRANSPORT="hostile") == DEFAULTS


def test_the_environment_is_read_in_knobs_h_only():
    found = []
    for root, dirs, files in os.walk(CSRC):
        dirs[:] = [d for d in dirs if not d.startswith("build")]      # the Makefile's object directories: no source there
        for f in files:
            path = os.path.join(root, f)
            if os.path.relpath(path, CSRC) == "knobs.h":
                continue
            with open(path, errors="replace") as fh:
                if "getenv" in fh.read():
                    found.append(os.path.relpath(path, CSRC))
    assert not found, f"getenv outside knobs.h: {found}"
