"""CPU: the C-ABI shared library builds / loads and exports every symbol include/instag_hip.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "instag_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(instag_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from instag_amd import _lib
    lib = _lib.lib()                       # builds with hipcc if missing; raises loudly otherwise
    names = _declared()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/instag_hip.h but not exported"
    assert set(names) == set(_lib.EXPORTED_SYMBOLS), set(names) ^ set(_lib.EXPORTED_SYMBOLS)
    assert lib.instag_abi_version() == _lib.ABI_VERSION == 10
    assert lib.instag_last_error() is not None


def test_struct_layout_matches_header():
    from instag_amd._lib import RasterArgs
    # 11 x 4-byte scalars (44 B) padded to 48, then 14 pointers (the last two: shs_rest, walk_hints)
    assert ctypes.sizeof(RasterArgs) == 48 + 14 * 8
    assert RasterArgs.bg.offset == 48 and RasterArgs.extra_attrs.offset == 48 + 11 * 8


def test_argument_errors_do_not_need_a_gpu():
    from instag_amd import _lib
    lib = _lib.lib()
    # NULL tensors / unsupported dimensions are rejected before any device work
    rc = lib.instag_sh_encode_forward(None, None, 4, 3, 4, None, None)
    assert rc != 0 and b"NULL" in lib.instag_last_error()
    one = ctypes.c_void_p(16)
    rc = lib.instag_sh_encode_forward(one, one, 4, 2, 4, None, None)
    assert rc != 0 and b"input dim == 3" in lib.instag_last_error()
    rc = lib.instag_grid_encode_forward(one, one, one, one, 4, 7, 1, 2, 0.5, 16, None, 0, 0, 0, None)
    assert rc != 0 and b"D must be" in lib.instag_last_error()


def test_grid_dispatch_errors_do_not_need_a_gpu():
    """The three grid entry points refuse a (D, C) outside the sixteen built instantiations and a level count outside
    [1, 64] with INSTAG_E_ARG, before any device work (the total variation: before its workspace is cleared)."""
    from instag_amd import _lib
    lib = _lib.lib()
    E_ARG = 1                                   # INSTAG_E_ARG, include/instag_hip.h
    one = ctypes.c_void_p(16)

    def forward(D, C, L):
        return lib.instag_grid_encode_forward(one, one, one, one, 4, D, C, L, 0.5, 16, None, 0, 0, 0, None)

    def backward(D, C, L):
        return lib.instag_grid_encode_backward(one, one, one, one, one, 4, D, C, L, 0.5, 16, None, None, 0, 0, 0, None)

    def total_variation(D, C, L):
        return lib.instag_grid_total_variation(one, one, one, one, 1e-3, 4, D, C, L, 0.5, 16, 0, 0, 8, one, 1 << 20, None)

    for call in (forward, backward, total_variation):
        for D, C in ((6, 2), (3, 3), (1, 1), (5, 16)):
            assert call(D, C, 2) == E_ARG, (call.__name__, D, C)
            assert b"D must be 2..5 and C must be 1, 2, 4, or 8" in lib.instag_last_error()
        for L in (0, 65):
            assert call(3, 2, L) == E_ARG, (call.__name__, L)
            assert b"L must be in [1,64]" in lib.instag_last_error()


def test_drop_in_package_names_import():
    import diff_gauss
    import gridencoder
    import shencoder
    assert diff_gauss.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")
    enc = gridencoder.GridEncoder(input_dim=2, num_levels=12, level_dim=1, base_resolution=16,
                                  log2_hashmap_size=17, desired_resolution=38.4)
    assert enc.output_dim == 12 and tuple(enc.embeddings.shape) == (9464, 1)
    assert shencoder.SHEncoder(3, 4).output_dim == 16
    from simple_knn._C import distCUDA2
    assert callable(distCUDA2)


def test_backend_module_names_import():
    """The module names the reference's own binding files look for first (gridencoder/grid.py:9-10,
    shencoder/sphere_harmonics.py:9-10) exist and export the pybind entry points of bindings.cpp."""
    import inspect
    import _gridencoder
    import _shencoder
    sigs = {
        (_gridencoder, "grid_encode_forward"): ["inputs", "embeddings", "offsets", "outputs", "B", "D", "C", "L", "S", "H",
                                                "dy_dx", "gridtype", "align_corners", "interp"],
        (_gridencoder, "grid_encode_backward"): ["grad", "inputs", "embeddings", "offsets", "grad_embeddings", "B", "D",
                                                 "C", "L", "S", "H", "dy_dx", "grad_inputs", "gridtype", "align_corners",
                                                 "interp"],
        (_gridencoder, "grad_total_variation"): ["inputs", "embeddings", "grad", "offsets", "weight", "B", "D", "C", "L",
                                                 "S", "H", "gridtype", "align_corners"],
        (_shencoder, "sh_encode_forward"): ["inputs", "outputs", "B", "D", "C", "dy_dx"],
        (_shencoder, "sh_encode_backward"): ["grad", "inputs", "B", "D", "C", "dy_dx", "grad_inputs"],
    }
    for (mod, name), params in sigs.items():
        assert list(inspect.signature(getattr(mod, name)).parameters) == params, name
