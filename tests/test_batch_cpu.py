"""CPU-only: the batched-ensemble ABI (include/nbody.h, nbody_batch_*) is declared, bound and exported by the product
library and by the RCCL test-double build; its header constant matches the Python mirror; bad arguments are refused
before any device work, and valid ones fail loudly without a device."""
import ctypes
import os
import re
import sys

import pytest

from conftest import ROOT

BATCH_NAMES = ["nbody_batch_create", "nbody_batch_destroy", "nbody_batch_last_error", "nbody_batch_set_counts",
               "nbody_batch_set_integrator", "nbody_batch_invalidate_forces", "nbody_batch_set_stream",
               "nbody_batch_step_n_on", "nbody_batch_step_n_async", "nbody_batch_sync", "nbody_batch_energy",
               "nbody_batch_momentum"]


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def header_text():
    return open(os.path.join(ROOT, "include", "nbody.h")).read()


def test_batch_entry_points_are_declared_bound_and_exported(lib):
    from n_body_problem_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    declared = set(re.findall(r"\b(nbody_batch_[a-z0-9_]+)\s*\(", code))
    assert declared == set(BATCH_NAMES)
    assert set(BATCH_NAMES) <= set(_lib.exported_names())
    for name in BATCH_NAMES:
        assert hasattr(lib, name), name
    sys.path.insert(0, os.path.join(ROOT, "tests", "fake_rccl"))
    import build_fake_rccl
    fake = ctypes.CDLL(build_fake_rccl.build())
    for name in BATCH_NAMES:
        assert hasattr(fake, name), name


def test_the_three_batch_sources_and_their_headers_are_build_dependencies_and_the_c_abi_source_holds_no_kernel():
    from n_body_problem_amd import build
    csrc = os.path.join(ROOT, "n_body_problem_amd", "csrc")
    text = {}
    for source in ("nbody_batch.hip", "nbody_batch_capi.hip", "nbody_batch_analysis.hip"):
        assert source in build.SOURCES
        text[source] = open(os.path.join(csrc, source)).read()
        for header in re.findall(r'^#include "([^"/]+)"', text[source], flags=re.M):
            assert os.path.join(csrc, header) in build.HEADERS, (source, header)
    assert os.path.join(csrc, "nbody_batch_launch.h") in build.HEADERS
    for source in ("nbody_batch.hip", "nbody_batch_capi.hip"):      # the two meet in that header
        assert '#include "nbody_batch_launch.h"' in text[source]
    host = re.sub(r"//[^\n]*", "", text["nbody_batch_capi.hip"])
    assert not re.search(r"__global__|__device__|hipLaunchKernelGGL|<<<|hipMalloc|hipFree", host)
    assert "nbody_batch_capi.hip" not in build.EXTRA_FLAGS          # no device code, no device flags
    assert 'extern "C"' not in text["nbody_batch.hip"]


def test_max_bodies_constant_matches_the_python_mirror():
    import n_body_problem_amd as nb
    from n_body_problem_amd import batch
    defines = dict(re.findall(r"^#define\s+(NBODY_[A-Z_]+)\s+(\d+)\s*$", header_text(), flags=re.M))
    assert int(defines["NBODY_BATCH_MAX_BODIES"]) == batch.BATCH_MAX_BODIES == nb.BATCH_MAX_BODIES == 4096
    assert int(defines["NBODY_ABI_VERSION"]) == 5          # the batch ABI is additive


def test_bad_arguments_are_refused_before_any_device_work(lib):
    from n_body_problem_amd import _lib
    INVALID = _lib.NBODY_ERR_INVALID
    h = ctypes.c_void_p(None)
    assert lib.nbody_batch_create(None, 0, 4, 64) == INVALID
    for n_systems, max_bodies, what in ((0, 64, b"n_systems"), (-3, 64, b"n_systems"), (4, 0, b"max_bodies"),
                                        (4, -1, b"max_bodies"), (4, 4097, b"max_bodies"), (1 << 31, 64, b"n_systems")):
        assert lib.nbody_batch_create(ctypes.byref(h), 0, n_systems, max_bodies) == INVALID
        assert not h.value and what in lib.nbody_batch_last_error(None)
    # every call on a NULL handle is an argument error, not a crash
    counts = (ctypes.c_int64 * 1)(1)
    out = (ctypes.c_double * 4)()
    assert lib.nbody_batch_set_counts(None, counts) == INVALID
    assert lib.nbody_batch_set_integrator(None, 1) == INVALID
    assert lib.nbody_batch_invalidate_forces(None) == INVALID
    assert lib.nbody_batch_set_stream(None, None) == INVALID
    assert lib.nbody_batch_step_n_on(None, None, None, 1, 0.01, 0.01) == INVALID
    assert lib.nbody_batch_step_n_async(None, None, None, 1, 0.01, 0.01) == INVALID
    assert lib.nbody_batch_sync(None) == INVALID
    assert lib.nbody_batch_energy(None, None, None, 0.01, out) == INVALID
    assert lib.nbody_batch_momentum(None, None, None, out) == INVALID
    assert lib.nbody_batch_destroy(None) == 0


def test_no_gpu_means_loud_failure_not_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    h = ctypes.c_void_p(None)
    for n_systems, max_bodies in ((1, 1), (1024, 1024), (16, 4096)):
        assert lib.nbody_batch_create(ctypes.byref(h), 0, n_systems, max_bodies) == _lib.NBODY_ERR_NO_DEVICE
        assert not h.value and b"no CPU path" in lib.nbody_batch_last_error(None)
    with pytest.raises(nb.NBodyError) as e:
        nb.BatchedSystem(8, 256)
    assert e.value.status == _lib.NBODY_ERR_NO_DEVICE
    with pytest.raises(nb.NBodyError) as e:
        nb.BatchedSystem(8, 5000)                      # argument errors come first, with or without a device
    assert e.value.status == _lib.NBODY_ERR_INVALID
    with pytest.raises(ValueError):
        nb.BatchedSystem(8, 256, integrator="leapfrog")


def test_the_cpp_wrapper_compiles(tmp_path):
    """include/nbody.hpp's nbody::Batch builds and links against the library (no device needed to compile)."""
    import subprocess
    from n_body_problem_amd import build
    build.build_library()
    src = tmp_path / "batch.cpp"
    src.write_text(r'''
#include "nbody.hpp"
#include <cstdio>
int main() {
    try {
        nbody::Batch b(16, 1024);
        b.kickDriftKick(true);
        std::printf("%lld\n", (long long)b.numSystems());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "batch"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
           "-L" + os.path.join(ROOT, "n_body_problem_amd"), "-lnbody_amd", "-L/opt/rocm/lib",
           "-Wl,-rpath," + os.path.join(ROOT, "n_body_problem_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
