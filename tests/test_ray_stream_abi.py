"""The device-resident ray queries (rt_intersect_rays_device,
rt_occluded_rays_device, rt_shade_rays_device) at the ABI level, without a
GPU: the header declares them, the ctypes mirror carries them, the library
exports them, all three say ABI version 7, and a null context is refused
before anything touches a device."""
import os
import re
import subprocess

from test_abi import HEADER, _declared_functions

NAMES = ("rt_intersect_rays_device", "rt_occluded_rays_device", "rt_shade_rays_device")


def test_declared_mirrored_and_exported(rt):
    declared = _declared_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", rt.abi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for n in NAMES:
        assert n in declared, n
        assert n in rt.abi.SIGNATURES, n
        assert n in exported, n
    # the ctypes signatures have the header's arities
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        args = re.search(n + r"\s*\(([^)]*)\)", src).group(1)
        assert len(rt.abi.SIGNATURES[n][1]) == len(args.split(",")), n


def test_abi_version_is_7(rt):
    hdr = open(HEADER).read()
    assert int(re.search(r"#define RT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7
    assert rt.abi.RT_ABI_VERSION == 7
    assert rt.load_library().rt_abi_version() == 7


def test_null_context_is_invalid(rt):
    """No device is needed to be told that there is no context."""
    lib = rt.load_library()
    a = rt.abi
    prm = rt.raytracing.params_struct()
    assert lib.rt_intersect_rays_device(None, None, 0, None) == a.RT_E_INVALID
    assert lib.rt_intersect_rays_device(None, 16, 1, 16) == a.RT_E_INVALID
    assert lib.rt_occluded_rays_device(None, None, None, 0, None) == a.RT_E_INVALID
    assert lib.rt_occluded_rays_device(None, 16, None, 1, 16) == a.RT_E_INVALID
    assert lib.rt_shade_rays_device(None, None, 0, prm, None, 0, None) == a.RT_E_INVALID
    assert lib.rt_shade_rays_device(None, 16, 1, prm, 16, 16, None) == a.RT_E_INVALID


def test_every_layer_names_the_three_calls():
    """Header, C# shim, C++ host mirror and INTEGRATION.md name the same calls."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for rel in (("bindings", "csharp", "RtNative.cs"), ("unity-raytracer_amd", "host", "RayTracer.hpp"),
                ("INTEGRATION.md",)):
        text = open(os.path.join(root, *rel)).read()
        for n in NAMES:
            assert n in text, (rel[-1], n)
