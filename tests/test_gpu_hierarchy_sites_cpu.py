"""The build sites of the GPU hierarchy builder (prosper_pt_set_gpu_hierarchy_sites), as far as no device
is needed: the binding's constants are the header's, the library exports both functions with the declared arguments, and
a null argument is refused before anything is touched."""
import ctypes as C
import os
import re

from prosper_amd import capi, structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "prosper_pt", "prosper_pt.h")).read()


def test_constants_match_the_header():
    text = _header()
    defines = {name: int(value) for name, value in re.findall(r"#define\s+PROSPER_PT_GPU_BUILD_SITE_(\w+)\s+(\d+)u", text)}
    assert defines == {"UPLOAD": S.GPU_BUILD_SITE_UPLOAD, "MESH_UPDATES": S.GPU_BUILD_SITE_MESH_UPDATES, "DRIFT": S.GPU_BUILD_SITE_DRIFT}
    assert sorted(defines.values()) == [1, 2, 4]  # a mask: one bit each
    assert re.search(r"#define\s+PROSPER_PT_ABI_VERSION\s+4\b", text)  # (the sites did not move the ABI version)


def test_library_has_both_functions_as_declared():
    text = _header()
    assert re.search(r"int\s+prosper_pt_set_gpu_hierarchy_sites\(prosper_pt_ctx \*ctx, uint32_t sites\);", text)
    assert re.search(r"int\s+prosper_pt_get_gpu_hierarchy_sites\(prosper_pt_ctx \*ctx, uint32_t \*sites\);", text)
    lib = capi.lib()
    assert lib.prosper_pt_set_gpu_hierarchy_sites.argtypes == [C.c_void_p, C.c_uint32]
    assert lib.prosper_pt_get_gpu_hierarchy_sites.argtypes == [C.c_void_p, C.POINTER(C.c_uint32)]
    assert callable(capi.Context.set_gpu_hierarchy_sites) and callable(capi.Context.gpu_hierarchy_sites)


def test_null_arguments_are_refused():
    lib = capi.lib()
    sites = C.c_uint32(5)
    assert lib.prosper_pt_set_gpu_hierarchy_sites(None, S.GPU_BUILD_SITE_UPLOAD) == -1 and b"null" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_get_gpu_hierarchy_sites(None, C.byref(sites)) == -1 and b"null" in lib.prosper_pt_last_error()
    assert sites.value == 5
