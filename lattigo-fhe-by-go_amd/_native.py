"""ctypes binding of include/lattigo_ring.h (liblattigo_ring_hip.so).

There is no CPU fallback: if the shared library is missing or no HIP device is visible,
every arithmetic entry point raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"``
or ``lattigo-fhe-by-go_amd/csrc/build.sh``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblattigo_ring_hip.so")

u64 = C.c_uint64
u64p = C.POINTER(C.c_uint64)
vp = C.c_void_p
i32 = C.c_int

STATUS = {0: "LR_OK", 1: "LR_ERR_INVALID_DEGREE", 2: "LR_ERR_NOT_NTT_FRIENDLY", 3: "LR_ERR_SHAPE",
          4: "LR_ERR_ARG", 5: "LR_ERR_HIP", 6: "LR_ERR_UNSUPPORTED", 7: "LR_ERR_NOMEM", 8: "LR_ERR_INTERNAL"}

class Options(C.Structure):
    """lr_options (include/lattigo_ring.h), field for field.  Options() is lr_options_init's image: every switch at its default."""
    _fields_ = [("struct_size", C.c_uint32), ("version", C.c_uint32)] + [(n, C.c_int32) for n in (
        "no_asm", "no_fp", "ntt_mode", "asm_variant", "asm14_1024", "no_wide14_small", "wide14_max_items", "ntt_split15", "split15_max_workgroups",
        "no_invfuse", "no_grid_padding", "ntt_stagger", "ntt_persist", "ntt_timeline", "no_epilogue", "no_int_epilogue", "rescale_unfused",
        "rescale_unpaired", "pair_max_workgroups", "ext_narrow", "ext_ieee_div", "no_ext_chunks", "no_staging", "no_exttop", "no_invtop",
        "no_ext_group", "keymac_narrow", "no_pair", "no_fork", "fork_below_workgroups", "bfv_no_ext_epilogue", "bfv_no_gather")] + [("bfv_gather_below", C.c_int64), ("bfv_encoder_unfused", C.c_int32), ("ckks_encoder_tiled", C.c_int32)]

    def __init__(self, **fields):
        super().__init__()
        check(lib().lr_options_init(C.byref(self)))
        for k, v in fields.items():
            if k not in dict(self._fields_):
                raise AttributeError("lr_options has no field %r" % k)
            setattr(self, k, int(v))

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BasisProduct(C.Structure):
    """lr_ckks_basis_product (include/lattigo_ring.h), field for field"""
    _fields_ = [(n, C.c_uint32) for n in ("n", "a", "b", "c")] + [(n, C.c_int32) for n in (
        "mul_level", "n_rescales", "level_after", "layer", "tail", "mult_side")] + [("scale_after", C.c_double)]


# every symbol declared in include/lattigo_ring.h: name -> argtypes
SYMBOLS = {
    "lr_last_error_string": [],
    "lr_device_count": [C.POINTER(i32)],
    "lr_build_info": [],
    "lr_options_init": [vp],
    "lr_context_get_options": [vp, vp],
    "lr_context_create": [u64, u64p, i32, i32, C.POINTER(vp)],
    "lr_context_create_ex": [u64, u64p, i32, i32, vp, C.POINTER(vp)],
    "lr_context_destroy": [vp],
    "lr_context_ntt_variants": [vp, C.POINTER(i32), C.POINTER(i32)],
    "lr_context_set_stream": [vp, vp],
    "lr_context_sync": [vp],
    "lr_context_info": [vp, u64p, C.POINTER(i32), C.POINTER(i32)],
    "lr_context_get_table": [vp, i32, u64p, C.c_size_t],
    "lr_poly_alloc": [vp, i32, i32, C.POINTER(vp)],
    "lr_poly_wrap": [vp, vp, i32, i32, C.POINTER(vp)],
    "lr_poly_wrap_strided": [vp, vp, i32, i32, C.c_longlong, C.POINTER(vp)],
    "lr_poly_free": [vp],
    "lr_poly_info": [vp, u64p, C.POINTER(i32), C.POINTER(i32), C.POINTER(vp)],
    "lr_poly_upload": [vp, i32, C.POINTER(u64p), i32],
    "lr_poly_download": [vp, i32, C.POINTER(u64p), i32],
    "lr_poly_upload_limb": [vp, i32, i32, vp],
    "lr_poly_download_limb": [vp, i32, i32, vp],
    "lr_ntt_host_limb": [vp, i32, i32, vp, vp],
    "lr_poly_unmarshal": [vp, i32, C.c_char_p, C.c_size_t],
    "lr_poly_marshal": [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)],
    "lr_poly_upload_dense": [vp, vp, C.c_size_t],
    "lr_poly_download_dense": [vp, vp, C.c_size_t],
    "lr_poly_zero": [vp],
    "lr_poly_set_limbs": [vp, i32],
    "lr_ntt": [vp, i32, vp, vp],
    "lr_intt": [vp, i32, vp, vp],
    "lr_ntt_limb": [vp, i32, vp, i32, vp, i32],
    "lr_intt_limb": [vp, i32, vp, i32, vp, i32],
    "lr_ntt_host": [vp, i32, C.POINTER(u64p), C.POINTER(u64p)],
    "lr_intt_host": [vp, i32, C.POINTER(u64p), C.POINTER(u64p)],
    "lr_ewise": [vp, i32, i32, vp, vp, vp, u64p],
    "lr_half_scalar_op": [vp, i32, i32, vp, vp, vp, vp],
    "lr_ckks_lincomb_constants": [vp, vp, i32, C.c_double, i32, C.c_double, i32, C.c_double, C.c_double, i32, vp, vp, vp, vp,
                                  C.POINTER(i32), C.POINTER(C.c_double), vp, vp, vp, vp, vp, vp],
    "lr_ckks_lincomb": [vp, i32, i32, C.POINTER(vp), C.POINTER(vp), vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_ckks_combine_constants": [vp, i32, i32, i32, i32, C.c_double, i32, i32, C.c_double, i32, i32, C.c_double, i32, C.POINTER(i32),
                                  C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(i32), vp],
    "lr_ckks_combine": [vp, i32, i32, i32, C.POINTER(vp), i32, C.POINTER(vp), i32, vp, vp, vp, vp, vp, vp, C.POINTER(vp)],
    "lr_permute_ntt": [vp, i32, vp, u64, vp],
    "lr_permute_ntt_index": [u64, u64, u64, u64p],
    "lr_permute": [vp, vp, u64, vp],
    "lr_mult_by_monomial": [vp, vp, u64, vp],
    "lr_shift": [vp, vp, u64, vp],
    "lr_rotate": [vp, vp, u64],
    "lr_simple_scaler_create": [vp, u64, C.POINTER(vp)],
    "lr_simple_scaler_destroy": [vp],
    "lr_simple_scaler_tables": [vp, u64p, C.POINTER(C.c_double), i32],
    "lr_simple_scale": [vp, vp, vp],
    "lr_bext_create": [vp, vp, C.POINTER(vp)],
    "lr_bext_destroy": [vp],
    "lr_modup_split_qp": [vp, i32, vp, vp],
    "lr_modup_split_pq": [vp, i32, vp, vp],
    "lr_moddown_ntt_pq": [vp, i32, vp, vp],
    "lr_moddown_split_ntt_pq": [vp, i32, vp, vp, vp],
    "lr_moddown_pq": [vp, i32, vp, vp],
    "lr_moddown_split_pq": [vp, i32, vp, vp, vp],
    "lr_moddown_split_qp": [vp, i32, i32, vp, vp, vp],
    "lr_bext_get_table": [vp, i32, u64p, C.c_size_t],
    "lr_decomposer_create": [vp, vp, C.POINTER(vp)],
    "lr_decomposer_destroy": [vp],
    "lr_decompose": [vp, i32, i32, vp, vp],
    "lr_decompose_and_split": [vp, i32, i32, vp, vp, vp],
    "lr_div_floor_by_last_modulus_ntt": [vp, vp],
    "lr_div_floor_by_last_modulus": [vp, vp],
    "lr_div_round_by_last_modulus_ntt": [vp, vp],
    "lr_div_round_by_last_modulus": [vp, vp],
    "lr_div_floor_by_last_modulus_many": [vp, vp, i32, i32],
    "lr_div_round_by_last_modulus_many": [vp, vp, i32, i32],
    "lr_ckks_plan_create": [vp, vp, i32, C.POINTER(vp)],
    "lr_ckks_plan_create_ex": [vp, vp, i32, vp, C.POINTER(vp)],
    "lr_ckks_plan_destroy": [vp],
    "lr_ckks_plan_stats": [vp, vp, vp],
    "lr_ckks_switch_keys": [vp, i32, vp, vp, vp, vp],
    "lr_bfv_switch_keys": [vp, vp, vp, vp, vp],
    "lr_bfv_relinearize": [vp, vp, vp, vp, vp, vp, vp],
    "lr_bfv_relinearize_deg": [vp, C.POINTER(vp), i32, C.POINTER(vp), vp, vp],
    "lr_bfv_rotate": [vp, vp, vp, u64, vp, vp, vp],
    "lr_bfv_rotate_chain": [vp, vp, vp, i32, u64p, C.POINTER(vp), i32, vp, vp],
    "lr_bfv_inner_sum": [vp, vp, vp, i32, C.POINTER(vp), vp, vp, vp],
    "lr_ckks_mulrelin": [vp, i32, vp, vp, vp, vp, vp, vp, vp],
    "lr_ckks_batcher_create": [vp, i32, vp],
    "lr_ckks_batcher_destroy": [vp],
    "lr_ckks_batcher_mulrelin": [vp, i32, vp, vp, vp, vp, vp, vp, vp],
    "lr_ckks_batcher_stats": [vp, vp, vp, vp],
    "lr_ckks_batcher_rotate": [vp, i32, vp, vp, C.c_uint64, vp, vp, vp],
    "lr_ckks_rescale": [vp, vp, vp],
    "lr_ckks_mul_norelin": [vp, i32, vp, vp, vp, vp, vp, vp, vp],
    "lr_ckks_mul_plain": [vp, i32, vp, vp, vp, vp, vp],
    "lr_ckks_encrypt_pk": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "lr_ckks_decrypt": [vp, i32, C.POINTER(vp), i32, vp, vp],
    "lr_context_last_ntt_kernel": [vp, C.c_char_p, C.c_size_t],
    "lr_context_timeline": [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)],
    "lr_selftest_division": [vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)],
    "lr_ckks_rotate": [vp, i32, vp, vp, u64, vp, vp, vp],
    "lr_ckks_rotate_chain": [vp, i32, vp, vp, i32, u64p, C.POINTER(vp), i32, vp, vp],
    "lr_ckks_power_basis_schedule": [vp, i32, C.c_double, i32, i32, C.c_double, i32, vp, i32, C.POINTER(i32), vp, vp, vp],
    "lr_ckks_power_basis": [vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, C.POINTER(vp), C.POINTER(vp)],
    "lr_ckks_rotate_hoisted": [vp, i32, vp, vp, i32, u64p, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)],
    "lr_bfv_plan_create": [vp, vp, u64, i32, C.POINTER(vp)],
    "lr_bfv_plan_create_ex": [vp, vp, u64, i32, vp, C.POINTER(vp)],
    "lr_bfv_plan_destroy": [vp],
    "lr_bfv_mul": [vp, vp, vp, vp, vp, vp, vp, vp],
    "lr_bfv_mul_deg": [vp, C.POINTER(vp), i32, C.POINTER(vp), i32, C.POINTER(vp)],
    "lr_bfv_batcher_create": [vp, vp, i32, vp],
    "lr_bfv_batcher_destroy": [vp],
    "lr_bfv_batcher_mul": [vp, vp, vp, vp, vp, vp, vp, vp],
    "lr_bfv_batcher_relinearize": [vp, vp, vp, vp, vp, vp, vp],
    "lr_bfv_batcher_stats": [vp, vp, vp, vp],
    "lr_bfv_encoder_create": [vp, u64, i32, C.POINTER(vp)],
    "lr_bfv_encoder_create_ex": [vp, u64, i32, vp, C.POINTER(vp)],
    "lr_bfv_encoder_destroy": [vp],
    "lr_bfv_encoder_tables": [vp, u64p, u64p],
    "lr_bfv_encoder_route": [vp, C.POINTER(i32)],
    "lr_bfv_encode_uint": [vp, vp, C.c_size_t, i32, vp],
    "lr_bfv_encode_int": [vp, vp, C.c_size_t, i32, vp],
    "lr_bfv_decode_uint": [vp, vp, i32, vp],
    "lr_bfv_decode_int": [vp, vp, i32, vp],
    "lr_bfv_encode_device": [vp, vp, C.c_size_t, i32, i32, vp],
    "lr_bfv_decode_device": [vp, vp, i32, i32, vp],
    "lr_bfv_encryptor_create": [vp, vp, i32, C.POINTER(vp)],
    "lr_bfv_encryptor_create_ex": [vp, vp, i32, vp, C.POINTER(vp)],
    "lr_bfv_encryptor_destroy": [vp],
    "lr_bfv_encrypt_pk": [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_bfv_encrypt_sk": [vp, i32, vp, vp, vp, vp, i32, vp, vp],
    "lr_bfv_encrypt_pk_device": [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_bfv_encrypt_sk_device": [vp, i32, vp, vp, vp, vp, i32, vp, vp],
    "lr_ckks_encryptor_create": [vp, vp, i32, C.POINTER(vp)],
    "lr_ckks_encryptor_create_ex": [vp, vp, i32, vp, C.POINTER(vp)],
    "lr_ckks_encryptor_destroy": [vp],
    "lr_ckks_encryptor_encrypt_pk": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_ckks_encryptor_encrypt_sk": [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp],
    "lr_ckks_encryptor_encrypt_pk_device": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_ckks_encryptor_encrypt_sk_device": [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp],
    "lr_keygen_create": [vp, vp, i32, C.POINTER(vp)],
    "lr_keygen_create_ex": [vp, vp, i32, vp, C.POINTER(vp)],
    "lr_keygen_destroy": [vp],
    "lr_keygen_secret_key": [vp, vp, vp, i32, vp],
    "lr_keygen_public_key": [vp, vp, vp, i32, vp, vp],
    "lr_keygen_switching_keys": [vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_keygen_relin_keys": [vp, vp, i32, vp, C.POINTER(vp)],
    "lr_keygen_rotation_keys": [vp, vp, u64p, i32, vp, C.POINTER(vp)],
    "lr_keygen_secret_key_device": [vp, vp, vp, i32, vp],
    "lr_keygen_public_key_device": [vp, vp, vp, i32, vp, vp],
    "lr_keygen_switching_keys_device": [vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_keygen_relin_keys_device": [vp, vp, i32, vp, C.POINTER(vp)],
    "lr_keygen_rotation_keys_device": [vp, vp, u64p, i32, vp, C.POINTER(vp)],
    "lr_collective_create": [vp, vp, i32, C.POINTER(vp)],
    "lr_collective_create_ex": [vp, vp, i32, vp, C.POINTER(vp)],
    "lr_collective_destroy": [vp],
    "lr_collective_ckks_cks_share": [vp, i32, vp, vp, vp, vp, i32, vp],
    "lr_collective_bfv_cks_share": [vp, vp, vp, vp, vp, i32, vp],
    "lr_collective_ckks_pcks_share": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_collective_bfv_pcks_share": [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_collective_ckks_cks_share_device": [vp, i32, vp, vp, vp, vp, i32, vp],
    "lr_collective_bfv_cks_share_device": [vp, vp, vp, vp, vp, i32, vp],
    "lr_collective_ckks_pcks_share_device": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_collective_bfv_pcks_share_device": [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_collective_aggregate": [vp, i32, vp, C.POINTER(vp), i32, vp],
    "lr_refresh_create": [vp, vp, u64, i32, C.POINTER(vp)],
    "lr_refresh_create_ex": [vp, vp, u64, i32, vp, C.POINTER(vp)],
    "lr_refresh_destroy": [vp],
    "lr_refresh_mask_words": [vp, i32, C.POINTER(i32)],
    "lr_refresh_ckks_shares": [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_refresh_ckks_shares_device": [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_refresh_ckks_recode": [vp, i32, vp, vp],
    "lr_refresh_ckks_finalize": [vp, i32, vp, vp, vp, vp],
    "lr_refresh_bfv_shares": [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_refresh_bfv_shares_device": [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp],
    "lr_refresh_bfv_finalize": [vp, vp, vp, vp, vp, vp, vp],
    "lr_refresh_aggregate": [vp, i32, C.POINTER(vp), i32, vp],
    "lr_setup_create": [vp, vp, i32, C.POINTER(vp)],
    "lr_setup_create_ex": [vp, vp, i32, vp, C.POINTER(vp)],
    "lr_setup_destroy": [vp],
    "lr_setup_ckg_share": [vp, vp, vp, vp, i32, vp],
    "lr_setup_ckg_share_device": [vp, vp, vp, vp, i32, vp],
    "lr_setup_rkg_round1": [vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_round1_device": [vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_round2": [vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_round2_device": [vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_round3": [vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_round3_device": [vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_key": [vp, vp, vp, vp],
    "lr_setup_rkg_naive_round1": [vp, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_naive_round1_device": [vp, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_naive_round2": [vp, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_naive_round2_device": [vp, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp)],
    "lr_setup_rkg_naive_key": [vp, vp, vp],
    "lr_setup_rtg_share": [vp, vp, u64p, i32, vp, vp, C.POINTER(vp)],
    "lr_setup_rtg_share_device": [vp, vp, u64p, i32, vp, vp, C.POINTER(vp)],
    "lr_setup_rtg_key": [vp, vp, vp, vp],
    "lr_setup_aggregate": [vp, C.POINTER(vp), i32, vp],
    "lr_bfv_decryptor_create": [vp, i32, C.POINTER(vp)],
    "lr_bfv_decryptor_destroy": [vp],
    "lr_bfv_decrypt": [vp, C.POINTER(vp), i32, vp, vp, i32],
    "lr_ckks_encoder_create": [vp, i32, vp, C.POINTER(vp)],
    "lr_ckks_encoder_create_ex": [vp, i32, vp, vp, C.POINTER(vp)],
    "lr_ckks_encoder_destroy": [vp],
    "lr_ckks_encoder_tables": [vp, u64p, vp],
    "lr_ckks_encoder_route": [vp, i32, C.POINTER(i32)],
    "lr_ckks_encode": [vp, vp, i32, i32, C.c_double, i32, vp],
    "lr_ckks_decode": [vp, vp, i32, i32, C.c_double, i32, vp],
    "lr_ckks_encode_device": [vp, vp, i32, i32, C.c_double, i32, vp],
    "lr_ckks_decode_device": [vp, vp, i32, i32, C.c_double, i32, vp],
    "lr_poly_copy_peer": [vp, vp, i32, vp, vp, i32, i32],
    "lr_context_wait_peer_copies": [vp],
    "lr_gather_blocks": [vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), i32],
    "lr_timer_start": [vp],
    "lr_timer_stop": [vp, C.POINTER(C.c_float)],
}

_lib = None


class LatticeRingError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (STATUS.get(code, code), msg))
        self.code = code


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("liblattigo_ring_hip.so is not built (%s); there is no CPU fallback -- run "
                           "__graft_entry__.build()" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, args in SYMBOLS.items():
        f = getattr(L, name)  # AttributeError if the header and the library disagree
        f.argtypes = args
        f.restype = C.c_char_p if name in ("lr_last_error_string", "lr_build_info") else i32
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = lib().lr_last_error_string()
        raise LatticeRingError(rc, msg.decode() if msg else "")
    return rc


def device_count():
    n = i32(0)
    try:
        check(lib().lr_device_count(C.byref(n)))
    except LatticeRingError:
        return 0
    return n.value
