"""Every render instantiation runs with DX10_CLAMP set (CPU only: reads the kernel
descriptors of the in-tree library).  vx_math.h's clamp01 is the hardware
clamp, which takes a NaN to 0 only under DX10_CLAMP; kernel_meta.check, which
build() runs, refuses a library without it, and the resource limits of
tests/test_kernel_resources.py are part of the same check."""
import pytest


@pytest.fixture(scope="module")
def lib(built):
    from voxmap_amd import build as vb
    return vb.OUT


def test_every_render_instantiation_has_dx10_clamp(lib):
    from voxmap_amd import kernel_meta
    modes = kernel_meta.descriptor_modes(lib)
    render = {kernel_meta.render_params(k): v for k, v in modes.items() if kernel_meta.render_params(k)}
    assert len(render) == 96                       # as tests/test_kernel_resources.py counts them
    for p, v in render.items():
        assert v.get("dx10_clamp") == 1, (p, v)
    # the 2D and query kernels pack or clamp too: the whole library is built alike
    assert all(v.get("dx10_clamp") == 1 for v in modes.values()), [k for k, v in modes.items() if v.get("dx10_clamp") != 1]


def test_check_still_holds_the_resource_limits(lib):
    """check() = the limits of tests/test_kernel_resources.py + the descriptor bit; it passes on the product."""
    from voxmap_amd import kernel_meta
    ks = kernel_meta.check(lib)
    assert sum(1 for k in ks if kernel_meta.render_params(k)) == 96
