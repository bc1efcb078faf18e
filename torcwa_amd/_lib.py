"""ctypes binding of libtrx.so (the gfx950 HIP library behind include/trx.h).

The product loads ONLY `torcwa_amd/libtrx.so` and fails loudly if it is missing: there is no CPU fallback.
`TrxLib(path)` is also used by the tests to bind the kernel-logic emulator build (tests/hipemu), which is test
infrastructure and never loaded from here.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_int, c_long, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtrx.so")

C64, C128 = 0, 1
OP_N, OP_T, OP_C = 0, 1, 2

_SIGS = {
    "trx_version": (c_int, []),
    "trx_strerror": (c_char_p, [c_int]),
    "trx_convmat_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "trx_convmat": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_convmat_orders_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "trx_convmat_orders": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    "trx_convmat_li_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "trx_convmat_li": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_size_t, c_void_p]),
    "trx_convmat_li_shapes_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "trx_convmat_li_shapes": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_double, c_double, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_convmat_li_shapes_backward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_double, c_double, c_int, c_int, c_int,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "trx_build_pq_aniso": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p]),
    "trx_build_a_aniso_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_build_a_aniso": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                  c_void_p]),
    "trx_normal_field_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "trx_normal_field": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_int, c_double, c_double, c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_convmat_nv_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "trx_convmat_nv": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_normal_field_lattice": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_convmat_nv_orders_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "trx_convmat_nv_orders": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_double, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_convmat_shapes_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "trx_convmat_shapes": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_double, c_int, c_void_p, c_int, c_int,
                                   c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_toeplitz_sums_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "trx_toeplitz_sums": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_convmat_shapes_backward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_double, c_int, c_int, c_int,
                                            c_void_p, c_void_p, c_void_p, c_void_p]),
    "trx_shape_normal_field": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "trx_shape_normal_field_backward_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "trx_shape_normal_field_backward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                                c_void_p, c_size_t, c_void_p]),
    "trx_convmat_nv_shapes_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "trx_convmat_nv_shapes": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_int,
                                      c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_void_p]),
    "trx_build_pq_tensor": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                    c_void_p, c_void_p]),
    "trx_build_a_tensor_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_build_a_tensor": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                   c_size_t, c_void_p]),
    "trx_gemm": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_long, c_void_p, c_int, c_long,
                         c_void_p, c_void_p, c_int, c_long, c_int, c_void_p]),
    "trx_lu_solve": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "trx_inverse_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_inverse": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_eig_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_build_pq": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "trx_layer_smatrix_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_layer_smatrix_ws_bytes_lean": (c_size_t, [c_int, c_int, c_int]),
    "trx_layer_smatrix": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_eig_backward_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_eig_backward": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_hmodes_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_hmodes": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_redheffer_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_redheffer": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_redheffer_halfspace_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "trx_redheffer_halfspace": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_redheffer_halfspace_columns_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "trx_redheffer_halfspace_columns": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                c_void_p, c_size_t, c_void_p]),
    "trx_build_a_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_build_a": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_matvec": (c_int, [c_int, c_void_p, c_void_p, c_long, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "trx_layer_flux_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "trx_layer_flux": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                               c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_layer_field": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                c_int, c_int, c_int, c_void_p, c_void_p]),
    "trx_field_synth": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                c_void_p, c_void_p]),
    "trx_modal_overlap_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "trx_modal_overlap": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_sym_fold_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "trx_sym_fold": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_sym_unfold": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "trx_sym_fold_backward": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "trx_sym_unfold_backward": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "trx_sym_fold_pair": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "trx_sym_fold_pair_bd": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "trx_sym_fold_pairs_backward": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                            c_void_p]),
    "trx_sym_fold_pair_bd_backward": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "trx_thickness_prepare_ws_bytes":(c_size_t, [c_int, c_int, c_int]),
    "trx_thickness_prepare": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_thickness_columns_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "trx_thickness_columns": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                      c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_thickness_columns_keep": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                           c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_thickness_columns_backward_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "trx_thickness_columns_backward": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                               c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_tuning": (c_int, [c_char_p, c_int]),
    "trx_prof_enable": (c_int, [c_int]),
    "trx_prof_reset": (c_int, []),
    "trx_prof_get": (c_int, [c_int, c_void_p]),
    "trx_prof_tag_name": (c_char_p, [c_int]),
    "trx_eig": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "trx_eig_last_fallback": (c_int, []),
    "trx_eig_ws_bytes_opts": (c_size_t, [c_int, c_int, c_int, ctypes.c_uint]),
    "trx_eig_opts": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, ctypes.c_uint]),
}


class TrxError(RuntimeError):
    pass


class TrxLib:
    """Typed handle on a libtrx build.  All pointer arguments are raw addresses (ints)."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise TrxError(
                f"{path} not found: the HIP extension is not built. Run `python torcwa_amd/csrc/build.py` "
                "(hipcc --offload-arch=gfx950). torcwa_amd has no CPU fallback.")
        self.path = path
        self.dll = ctypes.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(self.dll, name)      # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
            setattr(self, name[4:], fn)

    def check(self, rc):
        if rc != 0:
            raise TrxError(f"libtrx error {rc}: {self.strerror(rc).decode()}")


_lib = None


def lib() -> TrxLib:
    global _lib
    if _lib is None:
        _lib = TrxLib(LIB_PATH)
    return _lib


def exported_symbols():
    return sorted(_SIGS)
