"""Room on the CU for the sub-batch pipeline (csrc/orbx_extract.cpp run_chunk), read from the built code object: with
ORBX_FAST_ROOM=1 k_fast_rows is capped at ORBX_FAST_PIPE_WAVES waves per CU by its LDS request while the pipeline runs, and the
registers those waves leave free on every SIMD must hold pyramid waves of the other stream (without the cap FAST fills every
SIMD with 5 waves and the pyramid gets slots as FAST waves retire).  An edit that grows a kernel's register allocation or the
wave cap fails here, not in a profile."""
import os
import re
import subprocess
import tempfile

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb_slam2_detailed_comments_amd", "csrc")
VGPRS_PER_SIMD_LANE = 512    # gfx950: 512 VGPRs per lane of a SIMD, allocated in granules of 8
WAVES_PER_SIMD = 8           # wave slots of a SIMD
SIMDS_PER_CU = 4
PYR_BUDGET = 64              # register allocation of the pyramid kernels: two waves per SIMD beside four FAST waves


def _kernel_metadata(lib):
    """{kernel symbol: {field: value}} from the AMDHSA metadata note of the library's gfx950 code object"""
    tools = "/opt/rocm/lib/llvm/bin"
    objcopy, bundler, readelf = (os.path.join(tools, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))
    if not all(os.path.exists(t) for t in (objcopy, bundler, readelf)):
        pytest.skip("ROCm LLVM tools not found")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "gfx950.co")
        subprocess.check_call([objcopy, "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(d, "copy.so")])
        subprocess.check_call([bundler, "--unbundle", "--type=o", f"--input={fat}", f"--output={co}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for entry in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        entry = ".agpr_count:" + entry
        fields = dict(re.findall(r"\.(\w+):\s+(\S+)", entry))
        if "name" in fields and "vgpr_count" in fields:
            out[fields["name"]] = fields
    return out


def _alloc(fields):
    assert int(fields["agpr_count"]) == 0 and int(fields["private_segment_fixed_size"]) == 0, fields["name"]
    return (int(fields["vgpr_count"]) + 7) // 8 * 8


def _find(meta, name):
    hits = [v for k, v in meta.items() if re.match(rf"_Z\d+{name}\d", k)]
    assert len(hits) == 1, (name, list(meta))
    return hits[0]


def _header_int(name):
    src = open(os.path.join(CSRC, "orbx_internal.h")).read()
    m = re.search(rf"#define {name} \(?([0-9 *]+)\)?", src)
    return eval(m.group(1))


def test_fast_waves_leave_registers_for_the_pyramid(built_lib):
    meta = _kernel_metadata(built_lib)
    fast = _alloc(_find(meta, "k_fast_rows"))
    assert fast <= 96, f"k_fast_rows allocates {fast} VGPRs: fewer than 5 waves per SIMD even without the pipeline"
    waves = _header_int("ORBX_FAST_PIPE_WAVES")
    assert waves % SIMDS_PER_CU == 0
    fast_per_simd = waves // SIMDS_PER_CU
    free = VGPRS_PER_SIMD_LANE - fast_per_simd * fast
    for k in ("k_pyr_l0", "k_pyr_resize_rows"):
        a = _alloc(_find(meta, k))
        assert a <= PYR_BUDGET, f"{k} allocates {a} VGPRs (budget {PYR_BUDGET})"
        beside = min(free // a, WAVES_PER_SIMD - fast_per_simd)
        assert beside >= 2, f"{k}: {beside} waves per SIMD beside {fast_per_simd} FAST waves of {fast} VGPRs"


def test_lds_floor_caps_fast_at_the_pipeline_wave_count():
    """the LDS request of k_fast_rows in the pipeline (ORBX_LDS_PER_CU / ORBX_FAST_PIPE_WAVES bytes per one-wave workgroup)
    admits exactly that many waves per CU -- and the 640x480 kernel's own request (8 192 bytes, 20 waves) is below it"""
    lds, waves = _header_int("ORBX_LDS_PER_CU"), _header_int("ORBX_FAST_PIPE_WAVES")
    assert lds == 160 * 1024
    floor = lds // waves
    assert floor * waves <= lds < floor * (waves + 1)
    assert floor % 256 == 0          # no allocation granule rounds it up into one wave fewer
    own_vga = 8192                   # see orbx_launch_fast_rows: tile / score maps + work list + corner list at 640x480
    assert own_vga < floor and lds // own_vga == 20
    src = open(os.path.join(CSRC, "orbx_kernels.hip")).read()
    assert "(size_t)lds_floor > need ? (size_t)lds_floor : need" in src
