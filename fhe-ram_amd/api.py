"""Host-side mirror of the reference's public interface for the RAM path, over the C ABI.

Names, argument meaning and error behaviour follow /root/reference/src:
  Parameters              parameters.rs:147-287
  EvaluationKeysPrepared  keys.rs:27-71
  Address                 address.rs:21-119
  Ram                     ram.rs:25-294  (read :172, read_prepare_write :196, write :226)
The reference panics on misuse (assert!); here every failing call raises FheRamError carrying
the C-ABI status and the reference's message.

All ciphertext data crosses this boundary as numpy int64 arrays in Poulpy's host layouts
(include/fheram.h).  There is NO CPU implementation behind these classes: if the HIP library is
missing or no GPU is present, construction fails loudly.
"""
import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from .base import Base2D, get_base_2d

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

I64P = C.POINTER(C.c_int64)
builtins_list = list   # (RamBank.read_mix names its first group `list`)

READ_BATCH_MAX = 8   # FHERAM_READ_BATCH_MAX (include/fheram.h)
BANK_MAX = 8         # FHERAM_BANK_MAX
READ_LIST_MAX = 8    # FHERAM_READ_LIST_MAX
DERIVE_MAX = 8       # FHERAM_DERIVE_MAX
SELECT_BITS_MAX = 5  # FHERAM_SELECT_BITS_MAX
SELECT_MAX = 8       # FHERAM_SELECT_MAX
SRC_ZERO, SRC_HOST, SRC_MEMBER_RESULT, SRC_LIST_RESULT, SRC_SELECT_RESULT = 0, 1, 2, 3, 4   # FHERAM_SRC_*
SRC_REGS_RESULT, SRC_REGS_OLD = 5, 6   # FHERAM_SRC_REGS_RESULT / _REGS_OLD: a bank's register files
SRC_TABLE_RESULT = 8   # FHERAM_SRC_TABLE_RESULT: a bank's tables (kind 7 is unknown)
SRC_PEEK_RESULT = 10   # FHERAM_SRC_PEEK_RESULT: a bank's last peek or poke at public addresses (kinds 7 and 9 are unknown)
PEEK_MAX = 16          # FHERAM_PEEK_MAX
TABLE_BITS_MAX = 12             # FHERAM_TABLE_BITS_MAX
SELECTOR_WIDE_DIGITS_MAX = 5    # FHERAM_SELECTOR_WIDE_DIGITS_MAX
SELECT_FIELDS_MAX = 5   # FHERAM_SELECT_FIELDS_MAX
MIX_MAX = 8             # FHERAM_MIX_MAX
DERIVE_LIST_MAX = 32          # FHERAM_DERIVE_LIST_MAX
DERIVE_LIST_DIGITS_MAX = 64   # FHERAM_DERIVE_LIST_DIGITS_MAX
DERIVE_ADDRESS, DERIVE_SELECTOR, DERIVE_FIELD = 0, 1, 2   # FHERAM_DERIVE_ADDRESS / _SELECTOR / _FIELD
STATUS = {0: "OK", 1: "INVALID_ARG", 2: "STATE", 3: "UNINITIALIZED", 4: "KEYS", 5: "UNSUPPORTED", 6: "RANGE", 7: "DEVICE", 8: "PRECISION"}


class FheRamError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fheram status {code} ({STATUS.get(code, '?')}): {msg}")
        self.code = code
        self.msg = msg


class _CParams(C.Structure):
    _fields_ = [("log_n", C.c_uint32), ("base2k", C.c_uint32), ("rank", C.c_uint32), ("k_glwe_pt", C.c_uint32),
                ("k_glwe_ct", C.c_uint32), ("k_ggsw_addr", C.c_uint32), ("k_evk_trace", C.c_uint32),
                ("k_evk_ggsw_inv", C.c_uint32), ("word_size", C.c_uint32), ("n_decomp", C.c_uint32),
                ("decomp_n", C.c_uint8 * 16), ("max_addr", C.c_uint64)]


_CONFIG_FIELDS = ("limb_split", "fine_split", "memo", "pre_inv", "tail", "tail_test", "mid", "mid_test", "chain", "chain_y", "pair_z",
                  "fuse", "graph", "safe", "nco", "tail_ep", "monitor", "reserved")


class _CSelectSrc(C.Structure):
    """fheram_select_src (include/fheram.h): where a candidate word of a select comes from"""
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32)]


class _CSelectLane(C.Structure):
    """fheram_select_lane (include/fheram.h): GLWE `lane` of the word (kind, index)"""
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32), ("lane", C.c_int32), ("reserved", C.c_int32)]


class _CDeriveItem(C.Structure):
    """fheram_derive_item (include/fheram.h): one address, selector or selector field of a derive list"""
    _fields_ = [("kind", C.c_int32), ("first_bit", C.c_int32), ("sign", C.c_int32), ("field", C.c_int32), ("fu", C.c_void_p), ("target", C.c_void_p)]


class _CMixReads(C.Structure):
    """fheram_mix_reads (include/fheram.h): the three groups of a fheram_bank_read_mix"""
    _fields_ = [("members", C.POINTER(C.c_int)), ("addrs", C.POINTER(C.c_void_p)), ("n_list", C.c_int),
                ("tables", C.POINTER(C.c_void_p)), ("table_sels", C.POINTER(C.c_void_p)), ("n_table", C.c_int),
                ("regs", C.c_void_p), ("reg_sels", C.POINTER(C.c_void_p)), ("n_regs", C.c_int)]


class _CMixPrepares(C.Structure):
    """fheram_mix_prepares (include/fheram.h): the prepare list and the register file of a fheram_bank_read_prepare_write_mix"""
    _fields_ = [("members", C.POINTER(C.c_int)), ("addrs", C.POINTER(C.c_void_p)), ("n_list", C.c_int),
                ("regs", C.c_void_p), ("reg_sel", C.c_void_p)]


class _CConfig(C.Structure):
    """fheram_config (include/fheram.h): the execution switches of a context"""
    _fields_ = [(f, C.c_int32) for f in _CONFIG_FIELDS]


def library_path() -> str:
    # FHERAM_LIB selects an alternative build of the same HIP library (kernel-tuning experiments)
    return os.environ.get("FHERAM_LIB") or os.path.join(_HERE, "libfheram.so")


# every symbol include/fheram.h declares: (name, restype, argtypes)
_SYMBOLS = [
    ("fheram_params_default", C.c_int, [C.POINTER(_CParams)]),
    ("fheram_ctx_create", C.c_int, [C.POINTER(_CParams), C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_ctx_destroy", None, [C.c_void_p]),
    ("fheram_last_error", C.c_char_p, [C.c_void_p]),
    ("fheram_glwe_len", C.c_size_t, [C.c_void_p]),
    ("fheram_ggsw_len", C.c_size_t, [C.c_void_p]),
    ("fheram_atk_len", C.c_size_t, [C.c_void_p]),
    ("fheram_evk_inv_len", C.c_size_t, [C.c_void_p]),
    ("fheram_rows", C.c_size_t, [C.c_void_p]),
    ("fheram_n_digits", C.c_int, [C.c_void_p]),
    ("fheram_n_coordinates", C.c_int, [C.c_void_p]),
    ("fheram_keys_load", C.c_int, [C.c_void_p, I64P, C.c_int, C.POINTER(I64P), I64P, C.c_int64, I64P]),
    ("fheram_ram_upload", C.c_int, [C.c_void_p, I64P]),
    ("fheram_ram_download", C.c_int, [C.c_void_p, I64P]),
    ("fheram_ram_tree_download", C.c_int, [C.c_void_p, C.c_int, I64P]),
    ("fheram_ram_state", C.c_int, [C.c_void_p]),
    ("fheram_address_create", C.c_int, [C.c_void_p, C.POINTER(I64P), C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_address_destroy", None, [C.c_void_p]),
    ("fheram_read", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_read_batch", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, I64P]),
    ("fheram_read_prepare_write", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_write", C.c_int, [C.c_void_p, I64P, C.c_int, C.c_void_p]),
    ("fheram_word_stage", C.c_int, [C.c_void_p, I64P, C.c_int]),
    ("fheram_result_download", C.c_int, [C.c_void_p, I64P]),
    ("fheram_result_map", C.c_int, [C.c_void_p, C.POINTER(I64P)]),
    ("fheram_sync", C.c_int, [C.c_void_p]),
    ("fheram_roundoff_max", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("fheram_roundoff_reset", C.c_int, [C.c_void_p]),
    ("fheram_ctx_create_sharded", C.c_int, [C.POINTER(_CParams), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_config_default", None, [C.POINTER(_CConfig)]),
    ("fheram_ctx_create_cfg", C.c_int, [C.POINTER(_CParams), C.c_int, C.c_int, C.c_int, C.POINTER(_CConfig), C.POINTER(C.c_void_p)]),
    ("fheram_ctx_config", C.c_int, [C.c_void_p, C.POINTER(_CConfig)]),
    ("fheram_shard_info", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    ("fheram_stream_signal", C.c_int, [C.c_void_p, C.c_void_p]),
    ("fheram_stream_wait", C.c_int, [C.c_void_p, C.c_void_p]),
    ("fheram_write_begin", C.c_int, [C.c_void_p, C.c_void_p]),
    ("fheram_device_malloc", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("fheram_device_free", C.c_int, [C.c_void_p, C.c_void_p]),
    ("fheram_read_partial", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    ("fheram_read_finish", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, I64P]),
    ("fheram_write_root", C.c_int, [C.c_void_p, I64P, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    ("fheram_write_shard", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("fheram_glwe_external_product", C.c_int, [C.c_void_p, I64P, C.c_int, I64P, I64P]),
    ("fheram_glwe_automorphism", C.c_int, [C.c_void_p, C.c_int, C.c_int64, I64P, C.c_int, I64P]),
    ("fheram_glwe_trace", C.c_int, [C.c_void_p, C.c_int, C.c_int, I64P, C.c_int, I64P]),
    ("fheram_glwe_pack", C.c_int, [C.c_void_p, I64P, C.c_int, I64P]),
    ("fheram_ggsw_automorphism_inv", C.c_int, [C.c_void_p, I64P, I64P]),
    ("fheram_secret_create", C.c_int, [C.c_void_p, I64P, C.POINTER(C.c_void_p)]),
    ("fheram_secret_destroy", None, [C.c_void_p]),
    ("fheram_glwe_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, I64P, C.c_int, C.c_int, I64P, I64P, I64P]),
    ("fheram_glwe_decrypt", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, I64P, I64P]),
    ("fheram_ram_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, I64P, I64P]),
    ("fheram_address_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, I64P, I64P, C.POINTER(C.c_void_p)]),
    ("fheram_address_download", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_keys_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, I64P, I64P, I64P]),
    ("fheram_fheuint_ggsw_len", C.c_size_t, [C.c_void_p]),
    ("fheram_fheuint_create", C.c_int, [C.c_void_p, I64P, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_fheuint_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, I64P, I64P, C.POINTER(C.c_void_p)]),
    ("fheram_fheuint_download", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_fheuint_destroy", None, [C.c_void_p]),
    ("fheram_address_set_from_fheuint", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_address_alloc", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("fheram_address_derive", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_fheuint_create", C.c_int, [C.c_void_p, I64P, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_address_alloc", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("fheram_bank_address_derive", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_address_derive_at", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_address_derive_at", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_select_lanes", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.POINTER(_CSelectLane), I64P, I64P]),
    ("fheram_bank_selector_alloc_fields", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_selector_create_fields", C.c_int, [C.c_void_p, C.POINTER(I64P), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_selector_derive_fields", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    ("fheram_bank_selector_alloc", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_selector_create", C.c_int, [C.c_void_p, C.POINTER(I64P), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_selector_derive", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_selector_download", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_selector_n_digits", C.c_int, [C.c_void_p]),
    ("fheram_selector_destroy", None, [C.c_void_p]),
    ("fheram_bank_select", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.POINTER(_CSelectSrc), I64P, I64P]),
    ("fheram_bank_select_result", C.c_int, [C.c_void_p, C.c_int, C.c_int, I64P]),
    ("fheram_bank_write_list_selected", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]),
    ("fheram_bank_selftest_fail_select_alloc", C.c_int, [C.c_void_p, C.c_int]),
    ("fheram_bank_regs_create", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_regs_create_wide", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_regs_destroy", None, [C.c_void_p]),
    ("fheram_regs_bits", C.c_int, [C.c_void_p]),
    ("fheram_bank_regs_state", C.c_int, [C.c_void_p, C.c_void_p]),
    ("fheram_bank_regs_upload", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_bank_regs_download", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_bank_regs_pack", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(_CSelectSrc), I64P]),
    ("fheram_bank_regs_read", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, I64P]),
    ("fheram_bank_regs_result", C.c_int, [C.c_void_p, C.c_int, C.c_int, I64P]),
    ("fheram_bank_regs_read_prepare_write", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, I64P]),
    ("fheram_bank_regs_old_result", C.c_int, [C.c_void_p, I64P]),
    ("fheram_bank_regs_write", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _CSelectSrc, I64P]),
    ("fheram_bank_table_create", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_table_destroy", None, [C.c_void_p]),
    ("fheram_table_bits", C.c_int, [C.c_void_p]),
    ("fheram_bank_table_upload", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_bank_table_download", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_bank_table_load_plain", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t]),
    ("fheram_bank_table_read", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, I64P]),
    ("fheram_bank_table_result", C.c_int, [C.c_void_p, C.c_int, C.c_int, I64P]),
    ("fheram_bank_table_selector_alloc", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_table_selector_create", C.c_int, [C.c_void_p, C.POINTER(I64P), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_table_selector_alloc_fields", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_ram_load_plain", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]),
    ("fheram_bank_regs_load_plain", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t]),
    ("fheram_bank_peek", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.c_int, I64P]),
    ("fheram_bank_peek_result", C.c_int, [C.c_void_p, C.c_int, C.c_int, I64P]),
    ("fheram_bank_poke", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.c_int, C.POINTER(_CSelectSrc), I64P]),
    ("fheram_bank_regs_peek", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_int, I64P]),
    ("fheram_bank_regs_poke", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.POINTER(_CSelectSrc), I64P]),
    ("fheram_bank_selftest_fail_public_alloc", C.c_int, [C.c_void_p, C.c_int]),
    ("fheram_bank_read_mix", C.c_int, [C.c_void_p, C.POINTER(_CMixReads), I64P, I64P, I64P]),
    ("fheram_bank_read_prepare_write_mix", C.c_int, [C.c_void_p, C.POINTER(_CMixReads), C.POINTER(_CMixPrepares), I64P, I64P, I64P, I64P, I64P]),
    ("fheram_bank_secret_create", C.c_int, [C.c_void_p, I64P, C.POINTER(C.c_void_p)]),
    ("fheram_bank_keys_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, I64P, I64P, I64P]),
    ("fheram_bank_address_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, I64P, I64P, C.POINTER(C.c_void_p)]),
    ("fheram_bank_fheuint_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, I64P, I64P, C.POINTER(C.c_void_p)]),
    ("fheram_bank_glwe_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, I64P, C.c_int, C.c_int, I64P, I64P, I64P]),
    ("fheram_bank_glwe_decrypt", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, I64P, I64P]),
    ("fheram_bank_ram_encrypt_sk", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, I64P, I64P]),
    ("fheram_bank_regs_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, I64P, I64P]),
    ("fheram_bank_table_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, I64P, I64P]),
    ("fheram_bank_selector_encrypt_sk", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, I64P, I64P]),
    ("fheram_bank_source_decrypt", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_CSelectSrc), C.c_int, I64P, I64P, C.POINTER(C.c_double)]),
    ("fheram_bank_ram_decrypt", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    ("fheram_bank_regs_decrypt", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    ("fheram_bank_table_decrypt", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    ("fheram_timer_begin", C.c_int, [C.c_void_p]),
    ("fheram_timer_end", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("fheram_profile_enable", C.c_int, [C.c_void_p, C.c_int]),
    ("fheram_profile_get", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("fheram_tail_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("fheram_mid_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("fheram_mid_state", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    ("fheram_profile_reset", C.c_int, [C.c_void_p]),
    ("fheram_bench_external_product", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    ("fheram_bench_chain", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    ("fheram_device_info", C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]),
    ("fheram_group_create", C.c_int, [C.POINTER(_CParams), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_group_destroy", None, [C.c_void_p]),
    ("fheram_group_last_error", C.c_char_p, [C.c_void_p]),
    ("fheram_group_size", C.c_int, [C.c_void_p]),
    ("fheram_group_ctx", C.c_void_p, [C.c_void_p, C.c_int]),
    ("fheram_group_keys_load", C.c_int, [C.c_void_p, I64P, C.c_int, C.POINTER(I64P), I64P, C.c_int64, I64P]),
    ("fheram_group_ram_upload", C.c_int, [C.c_void_p, I64P]),
    ("fheram_group_ram_download", C.c_int, [C.c_void_p, I64P]),
    ("fheram_group_ram_tree_download", C.c_int, [C.c_void_p, C.c_int, I64P]),
    ("fheram_group_ram_state", C.c_int, [C.c_void_p]),
    ("fheram_group_address_create", C.c_int, [C.c_void_p, C.POINTER(I64P), C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_group_address_destroy", None, [C.c_void_p]),
    ("fheram_group_read", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_group_read_prepare_write", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_group_write", C.c_int, [C.c_void_p, I64P, C.c_int, C.c_void_p]),
    ("fheram_group_word_stage", C.c_int, [C.c_void_p, I64P, C.c_int]),
    ("fheram_group_result_download", C.c_int, [C.c_void_p, I64P]),
    ("fheram_group_peer_info", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    ("fheram_group_poisoned", C.c_int, [C.c_void_p]),
    ("fheram_group_roundoff_max", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("fheram_bank_create", C.c_int, [C.POINTER(_CParams), C.c_int, C.c_int, C.POINTER(_CConfig), C.POINTER(C.c_void_p)]),
    ("fheram_bank_destroy", None, [C.c_void_p]),
    ("fheram_bank_last_error", C.c_char_p, [C.c_void_p]),
    ("fheram_bank_size", C.c_int, [C.c_void_p]),
    ("fheram_bank_keys_load", C.c_int, [C.c_void_p, I64P, C.c_int, C.POINTER(I64P), I64P, C.c_int64, I64P]),
    ("fheram_bank_ram_upload", C.c_int, [C.c_void_p, C.c_int, I64P]),
    ("fheram_bank_ram_download", C.c_int, [C.c_void_p, C.c_int, I64P]),
    ("fheram_bank_ram_tree_download", C.c_int, [C.c_void_p, C.c_int, C.c_int, I64P]),
    ("fheram_bank_ram_state", C.c_int, [C.c_void_p, C.c_int]),
    ("fheram_bank_address_create", C.c_int, [C.c_void_p, C.POINTER(I64P), C.c_int, C.POINTER(C.c_void_p)]),
    ("fheram_bank_read", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), I64P]),
    ("fheram_bank_read_prepare_write", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), I64P]),
    ("fheram_bank_write", C.c_int, [C.c_void_p, C.c_int, C.c_int, I64P, C.POINTER(C.c_void_p)]),
    ("fheram_bank_result_download", C.c_int, [C.c_void_p, C.c_int, C.c_int, I64P]),
    ("fheram_bank_read_list", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int, I64P]),
    ("fheram_bank_read_list_result", C.c_int, [C.c_void_p, C.c_int, C.c_int, I64P]),
    ("fheram_bank_read_prepare_write_list", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int, I64P]),
    ("fheram_bank_write_list", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int, I64P]),
    ("fheram_bank_selftest_fail_list_alloc", C.c_int, [C.c_void_p, C.c_int]),
    ("fheram_bank_derive_list", C.c_int, [C.c_void_p, C.POINTER(_CDeriveItem), C.c_int]),
    ("fheram_bank_address_download", C.c_int, [C.c_void_p, C.c_void_p, I64P]),
    ("fheram_bank_sync", C.c_int, [C.c_void_p]),
    ("fheram_bank_roundoff_max", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("fheram_bank_roundoff_reset", C.c_int, [C.c_void_p]),
    ("fheram_bank_tail_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("fheram_bank_mid_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("fheram_bank_profile_enable", C.c_int, [C.c_void_p, C.c_int]),
    ("fheram_bank_profile_get", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("fheram_bank_profile_reset", C.c_int, [C.c_void_p]),
    ("fheram_selftest_convolve", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int]),
    ("fheram_selftest_convolve_rounded", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_double]),
    ("fheram_selftest_limb_forms", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("fheram_selftest_forms", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                        C.c_int, C.c_double, C.POINTER(C.c_double)]),
]


def exported_symbols() -> List[str]:
    return [s[0] for s in _SYMBOLS]


def library():
    """Load the HIP C-ABI library.  Fails loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise FheRamError(7, f"HIP extension missing: {path} not built (run __graft_entry__.build()); "
                                 "there is no CPU fallback")
        L = C.CDLL(path)
        lenient = bool(os.environ.get("FHERAM_LIB"))   # an experimental build named by FHERAM_LIB (A/B runs) may predate newer entry points
        for name, res, args in _SYMBOLS:
            if lenient and not hasattr(L, name):
                continue
            f = getattr(L, name)  # AttributeError if the .so does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def _p(a: np.ndarray):
    assert a.dtype == np.int64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(I64P)


def _i64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int64)


def galois_elements(log_n: int = 12) -> List[int]:
    """GLWE::trace_galois_elements (keys.rs:39,158): -1, then 5^(2^(i-1)) mod 2N."""
    two_n = 2 << log_n
    return [-1] + [pow(5, 1 << (i - 1), two_n) for i in range(1, log_n)]


class Parameters:
    """parameters.rs:147-176.  Defaults are the source constants (parameters.rs:11-21).  The layout factories of the
    reference are generic in every precision (parameters.rs:53-104); the kernels accept any precision inside the limb
    counts of its two published blocks (source constants and README.md:17-27)."""

    def __init__(self, max_addr: int = 1 << 14, decomp_n: Sequence[int] = (3, 3, 3, 3), word_size: int = 4,
                 k_glwe_pt: int = 3, k_glwe_ct: int = 51, k_ggsw_addr: int = 68, k_evk_trace: int = 68, k_evk_ggsw_inv: int = 85):
        self.log_n, self._base2k, self._rank = 12, 17, 1
        self._k_glwe_pt, self._k_glwe_ct, self._k_ggsw_addr = int(k_glwe_pt), int(k_glwe_ct), int(k_ggsw_addr)
        self._k_evk_trace, self._k_evk_ggsw_inv = int(k_evk_trace), int(k_evk_ggsw_inv)
        assert sum(decomp_n) == self.log_n  # parameters.rs:168
        self._max_addr, self._decomp_n, self._word_size = int(max_addr), [int(x) for x in decomp_n], int(word_size)

    @classmethod
    def new(cls):  # parameters.rs:167
        return cls()

    @classmethod
    def readme(cls, max_addr: int = 1 << 18, word_size: int = 4):
        """The parameter block of README.md:17-34, with which the published 450 ms / 1200 ms were taken:
        K_PT = 9, K_CT = 3*17, K_ADDR = 4*17, K_EVK = 5*17 for EVERY evaluation key (5-limb trace keys), MAX_ADDR = 2^18."""
        return cls(max_addr=max_addr, word_size=word_size, k_glwe_pt=9, k_evk_trace=85, k_evk_ggsw_inv=85)

    def n(self):
        return 1 << self.log_n

    def max_addr(self):  # parameters.rs:237
        return self._max_addr

    def basek(self):
        return self._base2k

    def rank(self):
        return self._rank

    def k_glwe_ct(self):
        return self._k_glwe_ct

    def k_glwe_pt(self):
        return self._k_glwe_pt

    def k_ggsw_addr(self):
        return self._k_ggsw_addr

    def k_evk_trace(self):
        return self._k_evk_trace

    def k_evk_ggsw_inv(self):
        return self._k_evk_ggsw_inv

    def word_size(self):
        return self._word_size

    def decomp_n(self):
        return list(self._decomp_n)

    def dnum_ct(self):  # parameters.rs:273-275
        return -(-self._k_glwe_ct // self._base2k)

    def dnum_ggsw(self):  # parameters.rs:277-279
        return -(-self._k_ggsw_addr // self._base2k)

    def base2d(self) -> Base2D:  # parameters.rs:285-287
        return get_base_2d(self._max_addr, self._decomp_n)

    def rows(self):
        return -(-self._max_addr // self.n())

    # element counts of the host layouts
    def glwe_len(self):
        return self.dnum_ct() * 2 * self.n()

    def ggsw_len(self):
        return self.dnum_ct() * 2 * self.dnum_ggsw() * 2 * self.n()

    def _c(self) -> _CParams:
        cp = _CParams()
        library().fheram_params_default(C.byref(cp))
        cp.k_glwe_pt, cp.k_glwe_ct, cp.k_ggsw_addr = self._k_glwe_pt, self._k_glwe_ct, self._k_ggsw_addr
        cp.k_evk_trace, cp.k_evk_ggsw_inv = self._k_evk_trace, self._k_evk_ggsw_inv
        cp.max_addr = self._max_addr
        cp.word_size = self._word_size
        cp.n_decomp = len(self._decomp_n)
        for i, d in enumerate(self._decomp_n):
            cp.decomp_n[i] = d
        return cp


class EvaluationKeysPrepared:
    """keys.rs:27-71.  Holds the std-form keys; `prepare` happens on the device when a Ram first
    uses them (fheram_keys_load)."""

    def __init__(self, gal_els: Sequence[int], atk_glwe, atk_ggsw_inv, tsk_ggsw_inv, atk_ggsw_inv_p: int = -1):
        self.gal_els = _i64(gal_els)
        self.atk_glwe = [_i64(k).ravel() for k in atk_glwe]
        self.atk_ggsw_inv = _i64(atk_ggsw_inv).ravel()
        self.tsk_ggsw_inv = _i64(tsk_ggsw_inv).ravel()
        self.atk_ggsw_inv_p = int(atk_ggsw_inv_p)

    @classmethod
    def from_dict(cls, evk: Dict):
        return cls(evk["gal_els"], list(evk["atk_glwe"]), evk["atk_ggsw_inv"], evk["tsk"])

    @classmethod
    def encrypt_sk(cls, ram: "Ram", sk: "GLWESecret", source_xa, source_xe, keep_std: bool = False):
        """EvaluationKeys::encrypt_sk (keys.rs:135-180) + prepare (keys.rs:57-71) on `ram`'s device.
        The sources stay on the host: source_xa.uniform_limbs(count), source_xe.gaussian(count, scale)
        are drawn in the reference's order (12 trace keys, tensor key, p = -1 key).  With keep_std the
        std forms come back too, so the keys can be loaded into other contexts."""
        p = ram.params
        n, b2k = p.n(), p.basek()
        s4, s5 = -(-p.k_evk_trace() // b2k), -(-p.k_evk_ggsw_inv() // b2k)
        n4, n5 = p.log_n * p.dnum_ct(), 2 * p.dnum_ggsw()
        mask = np.concatenate([source_xa.uniform_limbs(n4 * s4 * n), source_xa.uniform_limbs(n5 * s5 * n)])
        noise = np.concatenate([source_xe.gaussian(n4 * n, noise_scale(p.k_evk_trace(), b2k)),
                                source_xe.gaussian(n5 * n, noise_scale(p.k_evk_ggsw_inv(), b2k))])
        L = library()
        if isinstance(ram, RamBank):   # (fheram_bank_keys_encrypt_sk: the same keys from the same draws, on the bank)
            atk_len, inv_len = p.dnum_ct() * s4 * 2 * n, p.dnum_ggsw() * s5 * 2 * n
            fn = L.fheram_bank_keys_encrypt_sk
        else:
            atk_len, inv_len = L.fheram_atk_len(ram._h), L.fheram_evk_inv_len(ram._h)
            fn = L.fheram_keys_encrypt_sk
        std = np.zeros(p.log_n * atk_len + 2 * inv_len, dtype=np.int64) if keep_std else None
        ram._chk(fn(ram._h, sk._h, _p(mask), _p(noise), _p(std) if keep_std else None))
        gal = galois_elements(p.log_n)
        if keep_std:
            o = p.log_n * atk_len
            keys = cls(gal, [std[i * atk_len:(i + 1) * atk_len] for i in range(p.log_n)], std[o + inv_len:o + 2 * inv_len], std[o:o + inv_len])
        else:
            keys = cls.__new__(cls)
            keys.gal_els, keys.atk_glwe, keys.atk_ggsw_inv, keys.tsk_ggsw_inv, keys.atk_ggsw_inv_p = _i64(gal), None, None, None, -1
        ram._keys = keys   # already prepared on this context
        return keys


class Address:
    """address.rs:21-24: one Coordinate (list of GGSW digits) per Base1D of the plan."""

    def __init__(self, params: Parameters, ggsw_digits):
        self.base2d = params.base2d()
        n_digits = self.base2d.as_1d().size()
        self._digits = [_i64(g).ravel() for g in ggsw_digits]
        if len(self._digits) != n_digits:
            raise FheRamError(1, f"address needs {n_digits} GGSW digits, got {len(self._digits)}")
        self._handles = {}  # ctx handle -> device address

    @property
    def digits(self):
        """std-form GGSW digits on the host; an address encrypted on the device downloads them on first use"""
        if self._digits is None:
            h = next(iter(self._handles.values()))
            if isinstance(h.ram, RamBank):
                raise FheRamError(5, "the digits of an address derived on a bank stay on its device (the ABI has no bank form of fheram_address_download)")
            n_digits = self.base2d.as_1d().size()
            out = np.zeros((n_digits, h.ram.params.ggsw_len()), dtype=np.int64)
            h.ram._chk(library().fheram_address_download(h.ram._h, h.h, _p(out)))
            self._digits = [out[i] for i in range(n_digits)]
        return self._digits

    @classmethod
    def encrypt_sk(cls, ram: "Ram", value: int, sk: "GLWESecret", source_xa, source_xe):
        """Address::encrypt_sk (address.rs:86-109) on `ram`'s device with host-side sources (see
        EvaluationKeysPrepared.encrypt_sk).  The GGSW digits never touch the host unless `.digits` is read."""
        p = ram.params
        self = cls.__new__(cls)
        self.base2d = p.base2d()
        n_digits = self.base2d.as_1d().size()
        n, b2k = p.n(), p.basek()
        size = -(-p.k_ggsw_addr() // b2k)
        n_glwe = n_digits * p.dnum_ct() * 2
        mask = source_xa.uniform_limbs(n_glwe * size * n)
        noise = source_xe.gaussian(n_glwe * n, noise_scale(p.k_ggsw_addr(), b2k))
        out = C.c_void_p()
        fn = library().fheram_bank_address_encrypt_sk if isinstance(ram, RamBank) else library().fheram_address_encrypt_sk
        ram._chk(fn(ram._h, sk._h, int(value), _p(mask), _p(noise), C.byref(out)))
        self._digits = None
        self._handles = {id(ram): _AddrHandle(out.value, ram)}
        return self

    @classmethod
    def set_from_fheuint(cls, ram: "Ram", fheuint: "FheUintPrepared", sign: bool = True):
        """Address::set_from_fheuint (conversion.rs:68-82): every digit derived from the encrypted integer on the
        device.  sign=True: digits of X^{+digit} (what the reference's test decrypts to); sign=False: X^{-digit}, the
        convention of Address::encrypt_sk (address.rs:102-108), i.e. an address Ram.read accepts."""
        self = cls.__new__(cls)
        self.base2d = ram.params.base2d()
        out = C.c_void_p()
        ram._chk(library().fheram_address_set_from_fheuint(ram._h, fheuint._h, int(bool(sign)), C.byref(out)))
        self._digits = None
        self._handles = {id(ram): _AddrHandle(out.value, ram)}
        return self

    @classmethod
    def alloc(cls, owner):
        """an address on `owner`'s device (a Ram or a RamBank) with its buffers and no digits yet (fheram_address_alloc): what
        derive_addresses fills; read / write refuse it until then"""
        self = cls.__new__(cls)
        self.base2d = owner.params.base2d()
        out = C.c_void_p()
        fn = library().fheram_bank_address_alloc if isinstance(owner, RamBank) else library().fheram_address_alloc
        owner._chk(fn(owner._h, C.byref(out)))
        self._digits = None
        self._handles = {id(owner): _AddrHandle(out.value, owner)}
        return self

    @classmethod
    def alloc_from_params(cls, params: Parameters):  # address.rs:58
        glen = params.ggsw_len()
        return cls(params, [np.zeros(glen, dtype=np.int64) for _ in range(params.base2d().as_1d().size())])

    def n2(self):  # address.rs:113
        return len(self.base2d.v)

    def at(self, i):  # address.rs:117
        s = sum(b.size() for b in self.base2d.v[:i])
        return self.digits[s:s + self.base2d.v[i].size()]

    def _group(self, grp: "GroupRam"):
        h = self._handles.get(id(grp))
        if h is None:
            arr = (I64P * len(self.digits))(*[_p(d) for d in self.digits])
            out = C.c_void_p()
            grp._chk(library().fheram_group_address_create(grp._h, arr, len(self.digits), C.byref(out)))
            h = _GroupAddrHandle(out.value, grp)
            self._handles[id(grp)] = h
        return h.h

    def _bank(self, bank: "RamBank"):
        """the device address bound to `bank` (fheram_bank_address_create): one handle serves any of its members"""
        h = self._handles.get(id(bank))
        if h is None:
            arr = (I64P * len(self.digits))(*[_p(d) for d in self.digits])
            out = C.c_void_p()
            bank._chk(library().fheram_bank_address_create(bank._h, arr, len(self.digits), C.byref(out)))
            h = _AddrHandle(out.value, bank)
            self._handles[id(bank)] = h
        return h.h

    def _device(self, ram: "Ram"):
        h = self._handles.get(id(ram))
        if h is None:
            L = library()
            arr = (I64P * len(self.digits))(*[_p(d) for d in self.digits])
            out = C.c_void_p()
            ram._chk(L.fheram_address_create(ram._h, arr, len(self.digits), C.byref(out)))
            h = _AddrHandle(out.value, ram)
            self._handles[id(ram)] = h
        return h.h


class _GroupAddrHandle:
    def __init__(self, h, grp):
        self.h = h
        self.ram = grp

    def __del__(self):
        if self.h and _LIB is not None:
            _LIB.fheram_group_address_destroy(self.h)
            self.h = None


class FheUintPrepared:
    """poulpy-schemes' FheUintPrepared<u32> as the RAM path needs it (conversion.rs:68-82): one GGSW per bit of an
    encrypted integer, LSB first, on a Ram's device.  Layout: k = k_evk_ggsw_inv, 5 limbs, dnum 4 (include/fheram.h)."""

    def __init__(self, ram: "Ram", handle, n_bits):
        self.ram, self._h, self.n_bits = ram, handle, n_bits

    @classmethod
    def from_host(cls, ram, bits):
        """ram: a Ram, or a RamBank (fheram_bank_fheuint_create: an integer any member's addresses can be derived from)"""
        bits = _i64(bits)
        out = C.c_void_p()
        fn = library().fheram_bank_fheuint_create if isinstance(ram, RamBank) else library().fheram_fheuint_create
        ram._chk(fn(ram._h, _p(bits), bits.shape[0], C.byref(out)))
        return cls(ram, out.value, bits.shape[0])

    @classmethod
    def encrypt_sk(cls, ram: "Ram", value: int, sk: "GLWESecret", source_xa, source_xe, n_bits: int = 32):
        """FheUintPrepared::encrypt_sk (conversion.rs:160-168) with host-side sources, as the other encrypt_sk mirrors."""
        p = ram.params
        n, b2k, k = p.n(), p.basek(), p.k_evk_ggsw_inv()
        size = -(-k // b2k)
        n_glwe = n_bits * p.dnum_ggsw() * 2
        mask = source_xa.uniform_limbs(n_glwe * size * n)
        noise = source_xe.gaussian(n_glwe * n, noise_scale(k, b2k))
        out = C.c_void_p()
        fn = library().fheram_bank_fheuint_encrypt_sk if isinstance(ram, RamBank) else library().fheram_fheuint_encrypt_sk
        ram._chk(fn(ram._h, sk._h, int(value), n_bits, _p(mask), _p(noise), C.byref(out)))
        return cls(ram, out.value, n_bits)

    def download(self) -> np.ndarray:
        if isinstance(self.ram, RamBank):
            raise FheRamError(5, "an integer created on a bank stays on its device (the ABI has no bank form of fheram_fheuint_download)")
        out = np.zeros((self.n_bits, library().fheram_fheuint_ggsw_len(self.ram._h)), dtype=np.int64)
        self.ram._chk(library().fheram_fheuint_download(self.ram._h, self._h, _p(out)))
        return out

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.fheram_fheuint_destroy(self._h)
            self._h = None


def _derive_addresses(owner, fn, fheuints, addrs, sign, first_bits=None, fn_at=None):   # fn_at: the NAME of the _derive_at entry point (looked up only when used: a build named by FHERAM_LIB may predate it)
    """Ram.derive_addresses / RamBank.derive_addresses: addrs[i] <- Address::set_from_fheuint(fheuints[i]) as ONE launch; first_bits: the
    address bits start at bit first_bits[i] of integer i (fheram_address_derive_at: one launch per distinct first bit)"""
    fheuints = list(fheuints)
    k = len(fheuints)
    if first_bits is not None:
        first_bits = [int(f) for f in first_bits]
        if len(first_bits) != k:
            raise FheRamError(1, f"derive_addresses: {k} integers need {k} first bits")
    if not 1 <= k <= DERIVE_MAX:
        raise FheRamError(1, f"derive_addresses takes 1 to DERIVE_MAX = {DERIVE_MAX} integers, got {k}")
    if not all(isinstance(f, FheUintPrepared) for f in fheuints):
        raise FheRamError(1, "derive_addresses: every integer must be a FheUintPrepared")
    if addrs is None:
        addrs = [Address.alloc(owner) for _ in range(k)]
    else:
        addrs = list(addrs)
        if len(addrs) != k or not all(isinstance(a, Address) for a in addrs):
            raise FheRamError(1, f"derive_addresses: {k} integers need {k} Address objects")
    handles = [a._bank(owner) if isinstance(owner, RamBank) else a._device(owner) for a in addrs]   # (an address made from host digits: created here)
    fa, aa = (C.c_void_p * k)(*[f._h for f in fheuints]), (C.c_void_p * k)(*handles)
    if first_bits is None:
        owner._chk(fn(owner._h, fa, k, int(bool(sign)), aa))
    else:
        owner._chk(getattr(library(), fn_at)(owner._h, fa, (C.c_int * max(k, 1))(*first_bits), k, int(bool(sign)), aa))
    for a, f in zip(addrs, fheuints):
        a._digits = None                                               # the host copy, and the handles on other devices, held the old digits
        a._handles = {id(owner): a._handles[id(owner)]}
        a._derived_from = f                                            # the integer stays alive until the launch that reads it has run
    return addrs


class Derive:
    """One entry of RamBank.derive_list (fheram_derive_item): an address, a plain selector or the fields of a field selector, each from
    an encrypted integer, a first bit and (an address) a sign of its own.  Derive.fields gives one item per digit of its selector."""

    def __init__(self, kind: int, fu, target, first_bit: int = 0, sign: bool = False, field: int = 0):
        self.kind, self.fu, self.target, self.first_bit, self.sign, self.field = int(kind), fu, target, int(first_bit), bool(sign), int(field)

    @classmethod
    def address(cls, fu, addr=None, first_bit: int = 0, sign: bool = False):
        """addr <- the address read from bits [first_bit, ..) of fu; addr=None: derive_list allocates one (Address.alloc)"""
        if not isinstance(fu, FheUintPrepared) or not (addr is None or isinstance(addr, Address)):
            raise FheRamError(1, "Derive.address takes a FheUintPrepared and an Address (or None)")
        return cls(DERIVE_ADDRESS, fu, addr, first_bit, sign)

    @classmethod
    def selector(cls, fu, sel, first_bit: int = 0):
        """the plain selector sel <- bits [first_bit, first_bit + sel.bits) of fu"""
        if not isinstance(fu, FheUintPrepared) or not isinstance(sel, Selector) or sel.widths is not None:
            raise FheRamError(1, "Derive.selector takes a FheUintPrepared and a plain Selector (RamBank.selector, Selector.from_digits)")
        return cls(DERIVE_SELECTOR, fu, sel, first_bit)

    @classmethod
    def fields(cls, sel, fus, first_bits):
        """the field selector sel whole: digit d <- bits [first_bits[d], first_bits[d] + widths[d]) of fus[d]; a LIST of items"""
        if not isinstance(sel, Selector) or sel.widths is None:
            raise FheRamError(1, "Derive.fields takes a field selector (RamBank.selector_fields, Selector.from_digits_fields)")
        fus, first_bits = list(fus), [int(f) for f in first_bits]
        k = len(sel.widths)
        if len(fus) != k or len(first_bits) != k or not all(isinstance(f, FheUintPrepared) for f in fus):
            raise FheRamError(1, f"Derive.fields: a selector of {k} fields takes {k} FheUintPrepared and {k} first bits")
        return [cls(DERIVE_FIELD, fus[d], sel, first_bits[d], False, d) for d in range(k)]


class Src:
    """Where a candidate word of RamBank.select comes from (fheram_select_src): Src.member(m), Src.list(k), Src.select(k), Src.host(i), Src.zero()"""

    def __init__(self, kind: int, index: int = 0):
        self.kind, self.index = int(kind), int(index)

    @classmethod
    def zero(cls):
        """all-zero ciphertexts"""
        return cls(SRC_ZERO)

    @classmethod
    def host(cls, i: int):
        """slot i of the call's host_words"""
        return cls(SRC_HOST, i)

    @classmethod
    def member(cls, m: int):
        """member m's last read / read_prepare_write result"""
        return cls(SRC_MEMBER_RESULT, m)

    @classmethod
    def list(cls, k: int):
        """entry k of the last read list"""
        return cls(SRC_LIST_RESULT, k)

    @classmethod
    def select(cls, k: int):
        """output k of the previous select"""
        return cls(SRC_SELECT_RESULT, k)

    @classmethod
    def regs(cls, k: int):
        """output k of the bank's last RegFile.read"""
        return cls(SRC_REGS_RESULT, k)

    @classmethod
    def regs_old(cls):
        """the result of the bank's last RegFile.read_prepare_write: the word the pending register write replaces"""
        return cls(SRC_REGS_OLD, 0)

    @classmethod
    def table(cls, k: int):
        """output k of the bank's last RamBank.table_read"""
        return cls(SRC_TABLE_RESULT, k)

    @classmethod
    def peek(cls, k: int):
        """output k of the bank's last RamBank.peek (or the old word k of its last RamBank.poke)"""
        return cls(SRC_PEEK_RESULT, k)


class Lane:
    """One byte ciphertext of a lane-mapped candidate of RamBank.select_lanes (fheram_select_lane): GLWE `lane` of the word a Src would
    name.  Lane.zero(), Lane.host(i, lane), Lane.member(m, lane), Lane.list_entry(k, lane), Lane.select(k, lane)."""

    def __init__(self, kind: int, index: int = 0, lane: int = 0, reserved: int = 0):
        self.kind, self.index, self.lane, self.reserved = int(kind), int(index), int(lane), int(reserved)

    def __eq__(self, other):
        return isinstance(other, Lane) and (self.kind, self.index, self.lane, self.reserved) == (other.kind, other.index, other.lane, other.reserved)

    def __hash__(self):
        return hash((self.kind, self.index, self.lane, self.reserved))

    def __repr__(self):
        return f"Lane({self.kind}, {self.index}, {self.lane})"

    @classmethod
    def zero(cls):
        """an all-zero ciphertext"""
        return cls(SRC_ZERO)

    @classmethod
    def host(cls, i: int, lane: int):
        """GLWE `lane` of slot i of the call's host_words"""
        return cls(SRC_HOST, i, lane)

    @classmethod
    def member(cls, m: int, lane: int):
        """GLWE `lane` of member m's last read / read_prepare_write result"""
        return cls(SRC_MEMBER_RESULT, m, lane)

    @classmethod
    def list_entry(cls, k: int, lane: int):
        """GLWE `lane` of entry k of the last read list"""
        return cls(SRC_LIST_RESULT, k, lane)

    @classmethod
    def select(cls, k: int, lane: int):
        """GLWE `lane` of output k of the previous select"""
        return cls(SRC_SELECT_RESULT, k, lane)

    @classmethod
    def regs(cls, k: int, lane: int):
        """GLWE `lane` of output k of the bank's last RegFile.read"""
        return cls(SRC_REGS_RESULT, k, lane)

    @classmethod
    def regs_old(cls, lane: int):
        """GLWE `lane` of the result of the bank's last RegFile.read_prepare_write"""
        return cls(SRC_REGS_OLD, 0, lane)

    @classmethod
    def table(cls, k: int, lane: int):
        """GLWE `lane` of output k of the bank's last RamBank.table_read"""
        return cls(SRC_TABLE_RESULT, k, lane)

    @classmethod
    def peek(cls, k: int, lane: int):
        """GLWE `lane` of output k of the bank's last RamBank.peek / poke"""
        return cls(SRC_PEEK_RESULT, k, lane)

    @classmethod
    def of(cls, src: Src, lane: int):
        """GLWE `lane` of the word `src` names"""
        return cls.zero() if src.kind == SRC_ZERO else cls(src.kind, src.index, lane)


STORE_NONE, STORE_SB, STORE_SH, STORE_SW = 0, 1, 2, 3   # the `op` of store_merge_lanes (store.rs:87-142)
LOAD_LW, LOAD_LBU, LOAD_LHU = 0, 1, 2                   # the `op` of load_extract_lanes


def store_merge_lanes(x: Src, y: Src, word_size: int = 4):
    """The candidates of the reference's select_store (store.rs:87-142) in its order, as lanes of two words: x = the register's word (the
    bytes to store, from byte 0 up), y = the word the memory holds.  Candidate op + 4 * offset, op = NONE / SB / SH / SW, offset = the
    low address bits, is y with
        NONE  nothing replaced;
        SB    byte `offset` <- x0;
        SH    bytes offset, offset + 1 <- x0, x1    (offset 0 or 2);
        SW    every byte <- x                       (offset 0).
    The invalid combinations (a misaligned SH or SW) are all-ZERO candidates, and the two trailing ones (offset 3 with SH, SW) are left
    out: 14 candidates [14][word_size], for a selector of 4 bits.  An index of 14 or 15 then selects zero too.  No GPU work."""
    ws = int(word_size)
    if ws != 4:
        raise FheRamError(1, "store_merge_lanes restates the reference's 32-bit store merge: word_size = 4")
    Y = [Lane.of(y, w) for w in range(ws)]
    X = [Lane.of(x, w) for w in range(ws)]
    zero = [Lane.zero()] * ws
    out = []
    for offset in range(4):
        sb = list(Y)
        sb[offset] = X[0]
        if offset in (0, 2):
            sh = list(Y)
            sh[offset], sh[offset + 1] = X[0], X[1]
        else:
            sh = zero
        out += [list(Y), sb, sh, list(X) if offset == 0 else zero]
    return out[:14]


def load_extract_lanes(y: Src, word_size: int = 4):
    """The zero-extending loads as lanes of the word y the memory holds: candidate op + 4 * offset, op = LW / LBU / LHU (3: unused), is
        LW    [y0, y1, y2, y3]               (offset 0)
        LBU   [y_offset, 0, 0, 0]            (offset 0..3)
        LHU   [y_offset, y_offset+1, 0, 0]   (offset 0 or 2)
    and every other combination (a misaligned LW or LHU, op = 3) all ZERO; the trailing all-zero ones are left out: 14 candidates
    [14][word_size], for a selector of 4 bits.  It has NO reference counterpart (the reference's loads go through its un-vendored BDD
    circuits); sign-extending loads need bit operations inside a byte and are out of scope.  No GPU work."""
    ws = int(word_size)
    if ws != 4:
        raise FheRamError(1, "load_extract_lanes is the 32-bit load: word_size = 4")
    Y = [Lane.of(y, w) for w in range(ws)]
    Z = Lane.zero()
    zero = [Z] * ws
    out = []
    for offset in range(4):
        out += [list(Y) if offset == 0 else zero, [Y[offset], Z, Z, Z], [Y[offset], Y[offset + 1], Z, Z] if offset in (0, 2) else zero, zero]
    return out[:14]


class Selector:
    """The encrypted index of a select over up to 2^bits candidates (fheram_selector): the Address of a one-row RAM of max_addr = 2^bits on
    a bank's device.  RamBank.selector(bits) makes one without digits, Selector.from_digits one from host std-form GGSW digits;
    RamBank.derive_selectors fills either from bits of an encrypted integer.  A FIELD selector (RamBank.selector_fields,
    Selector.from_digits_fields; `widths` is set) has one digit per field, each filled from an integer and a bit position of its own by
    RamBank.derive_selector_fields."""

    def __init__(self, bank: "RamBank", handle, bits: int):
        self.bank, self._h, self.bits = bank, handle, int(bits)
        self.widths = None   # a field selector: the widths of its digits
        self._derived_from = None

    @classmethod
    def from_digits(cls, bank: "RamBank", bits: int, ggsw_digits):
        digits = [_i64(g).ravel() for g in ggsw_digits]
        arr = (I64P * max(len(digits), 1))(*[_p(d) for d in digits])
        out = C.c_void_p()
        bank._chk(library().fheram_bank_selector_create(bank._h, arr, len(digits), int(bits), C.byref(out)))
        return cls(bank, out.value, bits)

    @classmethod
    def from_digits_fields(cls, bank: "RamBank", widths, ggsw_digits):
        """a field selector (fheram_bank_selector_create_fields) from host std-form GGSW digits, one per field"""
        widths = [int(x) for x in widths]
        digits = [_i64(g).ravel() for g in ggsw_digits]
        arr = (I64P * max(len(digits), 1))(*[_p(d) for d in digits])
        out = C.c_void_p()
        bank._chk(library().fheram_bank_selector_create_fields(bank._h, arr, len(digits), (C.c_int * max(len(widths), 1))(*widths), len(widths), C.byref(out)))
        s = cls(bank, out.value, sum(widths))
        s.widths = widths
        return s

    def n_digits(self) -> int:
        return int(library().fheram_selector_n_digits(self._h))

    def encrypt_sk(self, value: int, sk: "GLWESecret", source_xa, source_xe):
        """fills this selector, in place, with Address::encrypt_sk's digits of `value` for the one-row RAM of max_addr = 2^bits over the
        handle's own plan (fheram_bank_selector_encrypt_sk); the sources draw in the address's order"""
        value = int(value)
        if not isinstance(sk, GLWESecret):
            raise FheRamError(1, "Selector.encrypt_sk takes a GLWESecret")
        if not 0 <= value < (1 << 32):   # (a value of 2^bits or more is the library's refusal, address.rs:98)
            raise FheRamError(1, f"Selector.encrypt_sk: {value} is not an unsigned 32-bit value")
        p = self.bank.params
        n, b2k = p.n(), p.basek()
        size = -(-p.k_ggsw_addr() // b2k)
        n_glwe = self.n_digits() * p.dnum_ct() * 2
        mask = source_xa.uniform_limbs(n_glwe * size * n)
        noise = source_xe.gaussian(n_glwe * n, noise_scale(p.k_ggsw_addr(), b2k))
        self.bank._chk(library().fheram_bank_selector_encrypt_sk(self.bank._h, sk._h, self._h, value, _p(mask), _p(noise)))
        self._derived_from = None

    def download(self) -> np.ndarray:
        """the std-form GGSW digits, [n_digits][ggsw_len]"""
        out = np.zeros((self.n_digits(), self.bank.params.ggsw_len()), dtype=np.int64)
        self.bank._chk(library().fheram_bank_selector_download(self.bank._h, self._h, _p(out)))
        return out

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.fheram_selector_destroy(self._h)
            self._h = None


class RegFile:
    """A register file of a bank (fheram_regs): a one-row RAM of 2^bits words of the bank's word_size that lives beside the members and is
    read and written by the bank's Selectors.  Made by RamBank.regfile(bits), bits <= SELECT_BITS_MAX, or WIDE by RamBank.scratch(bits),
    bits <= TABLE_BITS_MAX (up to 4096 words, addressed by RamBank.table_selector / table_selector_fields).  load / pack / load_plain /
    encrypt_sk make it readable; read runs several reads as one operation; read_prepare_write and write are the two halves of a register
    write, whose word comes from any Src; peek and poke read and write single words at PUBLIC indices."""

    def __init__(self, bank: "RamBank", handle, bits: int):
        self.bank, self._h, self.bits = bank, handle, int(bits)

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.fheram_regs_destroy(self._h)
            self._h = None

    def _row(self):
        p = self.bank.params
        return np.zeros((p.word_size(), p.glwe_len()), dtype=np.int64)

    def _sel(self, sel, what):
        if not isinstance(sel, Selector):
            raise FheRamError(1, f"RegFile.{what} takes a Selector")
        return sel

    def load(self, row: np.ndarray):
        """row: [word_size][GLWE], Ram::encrypt_sk's output for the one-row RAM of max_addr = 2^bits (fheram_bank_regs_upload)"""
        row = _i64(row)
        if row.size != self._row().size:
            raise FheRamError(1, f"invalid data: expected {self.bank.params.word_size()}x1 GLWE rows (ram.rs:144-155)")
        self.bank._chk(library().fheram_bank_regs_upload(self.bank._h, self._h, _p(row)))

    def encrypt_sk(self, data, sk: "GLWESecret", source_xa, source_xe):
        """Ram::encrypt_sk of the one-row RAM of max_addr = 2^bits, straight into the row (fheram_bank_regs_encrypt_sk).  data: 2^bits *
        word_size bytes, byte w of word j at data[j * word_size + w]; the sources draw in that small RAM's order."""
        self.bank._one_row_encrypt(library().fheram_bank_regs_encrypt_sk, self, self.bits, data, sk, source_xa, source_xe)

    def decrypt(self, sk: "GLWESecret"):
        """every word, decrypted and decoded on the device (fheram_bank_regs_decrypt): (values int32 [2^bits][word_size], worst log2 noise)"""
        return self.bank._one_row_decrypt(library().fheram_bank_regs_decrypt, self, self.bits, sk)

    def load_plain(self, data):
        """public contents, 2^bits * word_size bytes in Ram::encrypt_sk's layout (byte w of word j at data[j * word_size + w]), as the
        trivial ciphertext: no host encryption, no keys, no secret (fheram_bank_regs_load_plain)"""
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).ravel())
        want = (1 << self.bits) * self.bank.params.word_size()
        if data.size != want:
            raise FheRamError(1, f"invalid data: a register file of {self.bits} bits takes 2^bits * word_size = {want} bytes, got {data.size}")
        self.bank._chk(library().fheram_bank_regs_load_plain(self.bank._h, self._h, data.ctypes.data_as(C.POINTER(C.c_uint8)), data.size))

    def _public_entries(self, what, indices):
        indices = [int(i) for i in indices]
        n = len(indices)
        if not 1 <= n <= PEEK_MAX:
            raise FheRamError(1, f"RegFile.{what} takes 1 to PEEK_MAX = {PEEK_MAX} indices, got {n}")
        if n * self.bank.params.word_size() > 64:
            raise FheRamError(1, f"RegFile.{what}: n * word_size = {n * self.bank.params.word_size()} exceeds 64")
        for i in indices:
            if not 0 <= i < (1 << self.bits):
                raise FheRamError(1, f"RegFile.{what}: index {i} is outside the register file's 2^bits = {1 << self.bits} words")
        return n, indices

    def peek(self, indices, download: bool = True, keys: Optional["EvaluationKeysPrepared"] = None):
        """len(indices) reads at PUBLIC word indices as ONE operation (fheram_bank_regs_peek); indices may repeat.  int64
        [n][word_size][GLWE], each an encryption of [v, 0, .., 0]; download=False: no host wait (RamBank.peek_result later).  Nothing
        changes but the bank's last peek (Src.peek(k))."""
        n, indices = self._public_entries("peek", indices)
        if keys is not None:
            self.bank._use_keys(keys)
        p = self.bank.params
        out = np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64) if download else None
        self.bank._chk(library().fheram_bank_regs_peek(self.bank._h, self._h, (C.c_uint32 * n)(*indices), n, _p(out) if download else None))
        return out

    def poke(self, indices, words=None, srcs=None, keys: Optional["EvaluationKeysPrepared"] = None):
        """len(indices) writes at distinct PUBLIC word indices as ONE operation (fheram_bank_regs_poke).  Either words: int64
        [n][word_size][GLWE] host ciphertexts, entry k's at k — or srcs: one Src per entry, with words the host_words its Src.host(i)
        name.  Every entry sees the row as it was before the call; the OLD words are the bank's last peek afterwards
        (RamBank.peek_result, Src.peek(k)).  Never waits for the device."""
        n, indices = self._public_entries("poke", indices)
        if len(set(indices)) != n:
            raise FheRamError(1, "the targets of a poke are distinct indices")
        p = self.bank.params
        if srcs is None:
            if words is None:
                raise FheRamError(1, "poke takes words, or srcs")
            srcs = [Src.host(k) for k in range(n)]
            if _i64(words).size != n * p.word_size() * p.glwe_len():
                raise FheRamError(1, f"poke: expected {n} x {p.word_size()} GLWEs of words")
        srcs = list(srcs)
        if len(srcs) != n or not all(isinstance(s, Src) for s in srcs):
            raise FheRamError(1, f"poke takes one Src per entry, got {len(srcs)} for {n} entries")
        slots = [s.index for s in srcs if s.kind == SRC_HOST]
        if slots and words is None:
            raise FheRamError(1, "a host source needs words")
        if slots and max(slots) >= PEEK_MAX:
            raise FheRamError(1, f"a poke takes host slots [0, PEEK_MAX = {PEEK_MAX})")
        hw = self.bank._host_words(words, slots)
        if keys is not None:
            self.bank._use_keys(keys)
        arr = (_CSelectSrc * n)(*[_CSelectSrc(s.kind, s.index) for s in srcs])
        self.bank._chk(library().fheram_bank_regs_poke(self.bank._h, self._h, (C.c_uint32 * n)(*indices), n, arr, _p(hw) if hw is not None else None))

    def store(self) -> np.ndarray:
        """the row, [word_size][GLWE] (fheram_bank_regs_download)"""
        out = self._row()
        self.bank._chk(library().fheram_bank_regs_download(self.bank._h, self._h, _p(out)))
        return out

    def pack(self, sources, host_words=None):
        """row <- the pack of RamBank.select over `sources` (a list of 1..min(2^bits, 32) Src), word j at coefficient j (fheram_bank_regs_pack);
        [Src.zero()] * 2**bits is the all-zero register file"""
        sources = list(sources)
        if not sources or not all(isinstance(s, Src) for s in sources):
            raise FheRamError(1, "RegFile.pack takes a non-empty list of Src")
        hw = self.bank._host_words(host_words, [s.index for s in sources if s.kind == SRC_HOST])
        srcs = (_CSelectSrc * len(sources))(*[_CSelectSrc(s.kind, s.index) for s in sources])
        self.bank._chk(library().fheram_bank_regs_pack(self.bank._h, self._h, len(sources), srcs, _p(hw) if hw is not None else None))

    def read(self, sels, download: bool = True, keys: Optional["EvaluationKeysPrepared"] = None):
        """len(sels) reads of the register file as ONE operation (fheram_bank_regs_read): int64 [n][word_size][GLWE]; download=False: no
        host wait (RamBank.regs_result / RegFile.result later)"""
        sels = [self._sel(s, "read") for s in sels]
        n = len(sels)
        if n < 1:
            raise FheRamError(1, "RegFile.read takes at least one Selector")
        if keys is not None:
            self.bank._use_keys(keys)
        p = self.bank.params
        out = np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64) if download else None
        self.bank._chk(library().fheram_bank_regs_read(self.bank._h, self._h, (C.c_void_p * n)(*[s._h for s in sels]), n, _p(out) if download else None))
        return out

    def result(self, first: int = 0, n: int = 1) -> np.ndarray:
        """outputs [first, first + n) of the bank's last register read (fheram_bank_regs_result)"""
        first, n = int(first), int(n)
        p = self.bank.params
        out = np.zeros((max(n, 1), p.word_size(), p.glwe_len()), dtype=np.int64)
        self.bank._chk(library().fheram_bank_regs_result(self.bank._h, first, n, _p(out)))
        return out

    def read_prepare_write(self, sel, download: bool = True, keys: Optional["EvaluationKeysPrepared"] = None):
        """the first half of a register write (fheram_bank_regs_read_prepare_write): the OLD word, int64 [word_size][GLWE]; download=False:
        no host wait (old_result later)"""
        sel = self._sel(sel, "read_prepare_write")
        if keys is not None:
            self.bank._use_keys(keys)
        out = self._row() if download else None
        self.bank._chk(library().fheram_bank_regs_read_prepare_write(self.bank._h, self._h, sel._h, _p(out) if download else None))
        return out

    def old_result(self) -> np.ndarray:
        """the result of the bank's last register read_prepare_write (fheram_bank_regs_old_result)"""
        out = self._row()
        self.bank._chk(library().fheram_bank_regs_old_result(self.bank._h, _p(out)))
        return out

    def write(self, sel, src, host_words=None, keys: Optional["EvaluationKeysPrepared"] = None):
        """the second half (fheram_bank_regs_write): the word `src` names (any Src; Src.host(i): slot i of host_words) is written at the
        index read_prepare_write prepared.  Never waits for the device."""
        sel = self._sel(sel, "write")
        if not isinstance(src, Src):
            raise FheRamError(1, "RegFile.write takes the word as a Src")
        hw = self.bank._host_words(host_words, [src.index] if src.kind == SRC_HOST else [])
        if keys is not None:
            self.bank._use_keys(keys)
        self.bank._chk(library().fheram_bank_regs_write(self.bank._h, self._h, sel._h, _CSelectSrc(src.kind, src.index), _p(hw) if hw is not None else None))

    def state(self) -> bool:
        """True between read_prepare_write and write"""
        return bool(library().fheram_bank_regs_state(self.bank._h, self._h))


class Table:
    """A table of a bank (fheram_table): a READ-ONLY one-row RAM of 2^bits words, bits <= TABLE_BITS_MAX = 12, of the bank's word_size that
    lives beside the members and the register files — an instruction ROM, or a lookup table indexed by an encrypted field.  Made by
    RamBank.table(bits).  load (an encrypted row) or load_plain (public bytes, no host encryption) make it readable; RamBank.table_read
    reads any tables of the bank at wide Selectors (RamBank.table_selector) as one operation."""

    def __init__(self, bank: "RamBank", handle, bits: int):
        self.bank, self._h, self.bits = bank, handle, int(bits)

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.fheram_table_destroy(self._h)
            self._h = None

    def _row(self):
        p = self.bank.params
        return np.zeros((p.word_size(), p.glwe_len()), dtype=np.int64)

    def load(self, row: np.ndarray):
        """row: [word_size][GLWE], Ram::encrypt_sk's output for the one-row RAM of max_addr = 2^bits (fheram_bank_table_upload)"""
        row = _i64(row)
        if row.size != self._row().size:
            raise FheRamError(1, f"invalid data: expected {self.bank.params.word_size()}x1 GLWE rows (ram.rs:144-155)")
        self.bank._chk(library().fheram_bank_table_upload(self.bank._h, self._h, _p(row)))

    def encrypt_sk(self, data, sk: "GLWESecret", source_xa, source_xe):
        """Ram::encrypt_sk of the one-row RAM of max_addr = 2^bits, straight into the row (fheram_bank_table_encrypt_sk).  data: 2^bits *
        word_size bytes, byte w of word j at data[j * word_size + w]; the sources draw in that small RAM's order."""
        self.bank._one_row_encrypt(library().fheram_bank_table_encrypt_sk, self, self.bits, data, sk, source_xa, source_xe)

    def decrypt(self, sk: "GLWESecret"):
        """every word, decrypted and decoded on the device (fheram_bank_table_decrypt): (values int32 [2^bits][word_size], worst log2 noise)"""
        return self.bank._one_row_decrypt(library().fheram_bank_table_decrypt, self, self.bits, sk)

    def load_plain(self, data):
        """public contents, 2^bits * word_size bytes in Ram::encrypt_sk's layout (byte w of word j at data[j * word_size + w]), as the
        trivial ciphertext: no host encryption, no keys, no secret (fheram_bank_table_load_plain)"""
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).ravel())
        want = (1 << self.bits) * self.bank.params.word_size()
        if data.size != want:
            raise FheRamError(1, f"invalid data: a table of {self.bits} bits takes 2^bits * word_size = {want} bytes, got {data.size}")
        self.bank._chk(library().fheram_bank_table_load_plain(self.bank._h, self._h, data.ctypes.data_as(C.POINTER(C.c_uint8)), data.size))

    def download(self) -> np.ndarray:
        """the row, [word_size][GLWE] (fheram_bank_table_download)"""
        out = self._row()
        self.bank._chk(library().fheram_bank_table_download(self.bank._h, self._h, _p(out)))
        return out


class _AddrHandle:
    def __init__(self, h, ram):
        self.h = h
        self.ram = ram  # keeps the owning context alive for as long as the device address exists

    def __del__(self):
        if self.h and _LIB is not None:
            _LIB.fheram_address_destroy(self.h)
            self.h = None


def cast_u8_to_signed(value: int, bit_length: int) -> int:
    """examples/fhe-ram.rs:25-32"""
    shift = 8 - bit_length
    v = (value << shift) & 0xFF
    v = v - 256 if v >= 128 else v
    return v >> shift


def expected_plain(value: int, k_pt: int, written: bool = False) -> int:
    """cast_u8_to_signed generalised to any plaintext precision (README.md:20 has K_PT = 9, beyond the 8 bits the example's
    helper asserts): Ram::encrypt_sk encodes `(x as i8) as i64` (ram.rs:361-363), encrypt_glwe `value as i64`
    (examples/fhe-ram.rs:196); the torus keeps either mod 2^k_pt, centred."""
    v = int(value) if written else (int(value) - 256 if int(value) >= 128 else int(value))
    m = 1 << k_pt
    v %= m
    return v - m if v >= m // 2 else v


def encode_coeff(value: int, k: int, base2k: int = 17):
    """encode_coeff_i64(value, k, idx): value * 2^-k on ceil(k/base2k) normalised limbs"""
    size = -(-k // base2k)
    x = value << (size * base2k - k)
    limbs = [0] * size
    for j in range(size - 1, -1, -1):
        d = ((x + (1 << (base2k - 1))) % (1 << base2k)) - (1 << (base2k - 1))
        limbs[j] = d
        x = (x - d) >> base2k
    return limbs


def noise_scale(k: int, base2k: int = 17) -> float:
    """Noise of a ciphertext at precision k sits on limb ceil(k/base2k)-1, scaled by 2^((limb+1)*base2k - k)
    (Poulpy add_normal): the factor the host sampler multiplies sigma by."""
    return float(1 << (-(-k // base2k) * base2k - k))


class GLWESecret:
    """GLWESecret + GLWESecretPrepared (examples/fhe-ram.rs:49-59) on a Ram's or a RamBank's device: coefficients in {-1,0,1}."""

    def __init__(self, ram: "Ram", sk):
        self.ram = ram
        self._h = None
        out = C.c_void_p()
        fn = library().fheram_bank_secret_create if isinstance(ram, RamBank) else library().fheram_secret_create
        ram._chk(fn(ram._h, _p(_i64(sk)), C.byref(out)))
        self._h = out.value

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.fheram_secret_destroy(self._h)
            self._h = None


def _c_config(config: Optional[dict]):
    """fheram_config_default() with the switches of `config` set on top (fheram_config's field names); None for no config"""
    if not config:
        return None
    cfg = _CConfig()
    library().fheram_config_default(C.byref(cfg))
    for k, v in config.items():
        if k not in _CONFIG_FIELDS:
            raise FheRamError(1, f"unknown execution switch {k!r}")
        setattr(cfg, k, int(v))
    return cfg


class Ram:
    """ram.rs:25-29.  Owns the device-resident sub-RAMs, tree, packer scratch and prepared keys."""

    def __init__(self, params: Optional[Parameters] = None, device: int = 0, shard: int = 0, n_shards: int = 1, config: Optional[dict] = None):
        """shard / n_shards: row sharding across GPUs; this context then owns rows
        r = shard (mod n_shards) of every sub-RAM and only the *_partial / *_root / *_shard ops apply.
        config: execution switches that differ from fheram_config_default() (fheram_config's field names)."""
        self.params = params or Parameters.new()
        self.shard, self.n_shards = int(shard), int(n_shards)
        self._h = None
        L = library()
        out = C.c_void_p()
        cp = self.params._c()
        cfg = _c_config(config)
        if cfg is not None:
            rc = L.fheram_ctx_create_cfg(C.byref(cp), device, self.shard, self.n_shards, C.byref(cfg), C.byref(out))
        else:
            rc = L.fheram_ctx_create_sharded(C.byref(cp), device, self.shard, self.n_shards, C.byref(out))
        if rc != 0:
            raise FheRamError(rc, L.fheram_last_error(None).decode())
        self._h = out.value
        self._keys = None

    def forms(self) -> dict:
        """the execution switches in effect on this context (fheram_ctx_config)"""
        cfg = _CConfig()
        self._chk(library().fheram_ctx_config(self._h, C.byref(cfg)))
        return {f: int(getattr(cfg, f)) for f in _CONFIG_FIELDS if f != "reserved"}

    @classmethod
    def new(cls, device: int = 0):  # ram.rs:59
        return cls(Parameters.new(), device)

    @classmethod
    def new_from_ram_params(cls, word_size: int, decomp_n: Sequence[int], max_addr: int, device: int = 0, **crypto):  # ram.rs:72
        """crypto: k_glwe_pt / k_evk_trace / ... (CryptographicParameters, parameters.rs:23-32), default = source constants"""
        return cls(Parameters(max_addr=max_addr, decomp_n=decomp_n, word_size=word_size, **crypto), device)

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.fheram_ctx_destroy(self._h)
            self._h = None

    def _chk(self, rc):
        if rc != 0:
            raise FheRamError(rc, library().fheram_last_error(self._h).decode())

    def _use_keys(self, keys: EvaluationKeysPrepared):
        if self._keys is keys:
            return
        if keys.atk_glwe is None:
            raise FheRamError(5, "these keys were generated on another context's device (EvaluationKeysPrepared.encrypt_sk "
                                 "without keep_std=True): their std forms are not on the host")
        L = library()
        atk_len, inv_len = L.fheram_atk_len(self._h), L.fheram_evk_inv_len(self._h)
        if any(k.size != atk_len for k in keys.atk_glwe) or keys.atk_ggsw_inv.size != inv_len or keys.tsk_ggsw_inv.size != inv_len:
            raise FheRamError(1, f"evaluation-key layout does not match the context's (trace keys of {atk_len} limbs-elements, "
                                 f"inverse / tensor keys of {inv_len}: evk_glwe_infos / evk_ggsw_infos, parameters.rs:71-93)")
        arr = (I64P * len(keys.atk_glwe))(*[_p(k) for k in keys.atk_glwe])
        self._chk(L.fheram_keys_load(self._h, _p(keys.gal_els), len(keys.gal_els), arr, _p(keys.atk_ggsw_inv),
                                     keys.atk_ggsw_inv_p, _p(keys.tsk_ggsw_inv)))
        self._keys = keys

    def _out(self):
        return np.zeros((self.params.word_size(), self.params.glwe_len()), dtype=np.int64)

    # -- data hand-over (Ram::encrypt_sk output, ram.rs:129-167)
    def local_rows(self) -> int:
        return self.params.rows() // self.n_shards

    def load_encrypted(self, rows: np.ndarray):
        """rows: [word_size][rows][GLWE]; a sharded context takes its own rows (rows[:, shard::n_shards])."""
        p = self.params
        rows = _i64(rows)
        if rows.size != p.word_size() * self.local_rows() * p.glwe_len():
            raise FheRamError(1, f"invalid data: expected {p.word_size()}x{self.local_rows()} GLWE rows (ram.rs:144-155)")
        self._chk(library().fheram_ram_upload(self._h, _p(rows)))

    def encrypt_sk(self, data, sk: GLWESecret, source_xa, source_xe):
        """Ram::encrypt_sk (ram.rs:129-167) on the device.  data: max_addr*word_size bytes.  The sources are
        host objects (uniform_limbs(count) / gaussian(count, scale)); draws are made for every row of the
        RAM in the reference's order and a sharded context keeps those of its own rows."""
        p = self.params
        data = np.ascontiguousarray(data, dtype=np.uint8).ravel()
        n, b2k = p.n(), p.basek()
        size = -(-p.k_glwe_ct() // b2k)
        ws, rows = p.word_size(), p.rows()
        mask = source_xa.uniform_limbs(ws * rows * size * n).reshape(ws, rows, size * n)
        noise = source_xe.gaussian(ws * rows * n, noise_scale(p.k_glwe_ct(), b2k)).reshape(ws, rows, n)
        if self.n_shards > 1:
            mask = np.ascontiguousarray(mask[:, self.shard::self.n_shards])
            noise = np.ascontiguousarray(noise[:, self.shard::self.n_shards])
        self._chk(library().fheram_ram_encrypt_sk(self._h, sk._h, data.ctypes.data_as(C.POINTER(C.c_uint8)), data.size,
                                                  _p(mask), _p(noise)))

    def glwe_encrypt_sk(self, sk: GLWESecret, n_glwe: int, size: int, k: int, pt, pt_col: int, source_xa, source_xe):
        """GLWE::encrypt_sk on n_glwe ciphertexts (examples/fhe-ram.rs:179-210); pt [n_glwe][pt_size][N] or None."""
        n = self.params.n()
        mask = source_xa.uniform_limbs(n_glwe * size * n)
        noise = source_xe.gaussian(n_glwe * n, noise_scale(k, self.params.basek()))
        out = np.zeros((n_glwe, size * 2 * n), dtype=np.int64)
        pt_size = 0
        if pt is not None:
            pt = _i64(pt).reshape(n_glwe, -1, n)
            pt_size = pt.shape[1]
        self._chk(library().fheram_glwe_encrypt_sk(self._h, sk._h, n_glwe, size, k, _p(pt) if pt is not None else None,
                                                   pt_size, pt_col, _p(mask), _p(noise), _p(out)))
        return out

    def glwe_decrypt(self, sk: GLWESecret, cts, size: int = 3):
        """GLWE::decrypt (examples/fhe-ram.rs:217-222): normalised plaintext limbs [n_glwe][size][N]."""
        n = self.params.n()
        cts = _i64(cts).reshape(-1, size * 2 * n)
        pt = np.zeros((cts.shape[0], size, n), dtype=np.int64)
        self._chk(library().fheram_glwe_decrypt(self._h, sk._h, cts.shape[0], size, _p(cts), _p(pt)))
        return pt

    def encrypt_word(self, sk: GLWESecret, values, source_xa, source_xe):
        """encrypt_glwe of the example (examples/fhe-ram.rs:179-210): one GLWE per byte, value on coefficient 0
        at precision k_pt."""
        p = self.params
        values = [int(v) for v in values]
        size_pt = -(-p.k_glwe_pt() // p.basek())
        pt = np.zeros((len(values), size_pt, p.n()), dtype=np.int64)
        for i, v in enumerate(values):
            pt[i, :, 0] = encode_coeff(v, p.k_glwe_pt(), p.basek())
        return self.glwe_encrypt_sk(sk, len(values), -(-p.k_glwe_ct() // p.basek()), p.k_glwe_ct(), pt, 0, source_xa, source_xe)

    def decrypt_coeff(self, sk: GLWESecret, cts, wants, coeff: int = 0):
        """decrypt_glwe + noise metric of the example (examples/fhe-ram.rs:212-237) for each ct:
        returns [(value, log2 noise)]."""
        p = self.params
        k, b2k = p.k_glwe_ct(), p.basek()
        size = -(-k // b2k)
        pt = self.glwe_decrypt(sk, cts, size)
        out = []
        for limbs, want in zip(pt[:, :, coeff], wants):
            res = 0
            rem = b2k - (k % b2k)
            for j in range(size):                       # decode_coeff_i64(k, coeff)
                x = int(limbs[j])
                res = (res << (b2k - rem)) + (x >> rem) if (j == size - 1 and rem != b2k) else (res << b2k) + x
            log_scale = k - p.k_glwe_pt()                # :228
            diff = res - (int(want) << log_scale)        # :230
            noise = float(np.log2(abs(diff))) - k if diff != 0 else float("-inf")   # :231
            mag = int(np.floor(abs(res) / (1 << log_scale) + 0.5))   # round half away from zero  :232-233
            out.append((mag if res >= 0 else -mag, noise))
        return out

    def store_encrypted(self) -> np.ndarray:
        p = self.params
        rows = np.zeros((p.word_size(), self.local_rows(), p.glwe_len()), dtype=np.int64)
        self._chk(library().fheram_ram_download(self._h, _p(rows)))
        return rows

    def tree(self, level: int = 0) -> np.ndarray:
        out = self._out()
        self._chk(library().fheram_ram_tree_download(self._h, level, _p(out)))
        return out

    @property
    def state(self) -> bool:
        return bool(library().fheram_ram_state(self._h))

    # -- the path
    def _check_out(self, out):
        """a caller-owned result buffer is written by the library (word_size * GLWE int64): refuse anything it could overrun"""
        p = self.params
        if not (isinstance(out, np.ndarray) and out.dtype == np.int64 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
                and out.size == p.word_size() * p.glwe_len()):
            raise FheRamError(1, f"out must be a writeable C-contiguous int64 array of {p.word_size()} x {p.glwe_len()} elements")

    def read(self, address: Address, keys: EvaluationKeysPrepared, download: bool = True, out=None):  # ram.rs:172
        """out: an int64 array [word_size][GLWE] to receive the result (a host that reads in a loop reuses one)"""
        self._use_keys(keys)
        if download and out is None:
            out = self._out()
        elif download:
            self._check_out(out)
        self._chk(library().fheram_read(self._h, address._device(self), _p(out) if download else None))
        return out if download else None

    def read_batch(self, addresses, keys: EvaluationKeysPrepared, download: bool = True, out=None):  # ram.rs:172, K times
        """K = len(addresses) independent reads of this RAM as one operation (fheram_read_batch): int64 [K][word_size][GLWE],
        slice i equal to read(addresses[i]).  1 <= K <= READ_BATCH_MAX; duplicates are allowed.  out: an int64 array of that
        shape to receive the results (reused like read's)."""
        addresses = list(addresses)
        if not 1 <= len(addresses) <= READ_BATCH_MAX:
            raise FheRamError(1, f"read_batch takes 1 to {READ_BATCH_MAX} addresses, got {len(addresses)}")
        if not all(isinstance(a, Address) for a in addresses):
            raise FheRamError(1, "read_batch: every entry must be an Address")
        self._use_keys(keys)
        p = self.params
        k = len(addresses)
        if download and out is None:
            out = np.zeros((k, p.word_size(), p.glwe_len()), dtype=np.int64)
        elif download:
            if not (isinstance(out, np.ndarray) and out.dtype == np.int64 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
                    and out.size == k * p.word_size() * p.glwe_len()):
                raise FheRamError(1, f"out must be a writeable C-contiguous int64 array of {k} x {p.word_size()} x {p.glwe_len()} elements")
        arr = (C.c_void_p * k)(*[a._device(self) for a in addresses])
        self._chk(library().fheram_read_batch(self._h, arr, k, _p(out) if download else None))
        return out if download else None

    def read_prepare_write(self, address: Address, keys: EvaluationKeysPrepared, download: bool = True, out=None):  # ram.rs:196
        self._use_keys(keys)
        if download and out is None:
            out = self._out()
        elif download:
            self._check_out(out)
        self._chk(library().fheram_read_prepare_write(self._h, address._device(self), _p(out) if download else None))
        return out if download else None

    def derive_addresses(self, fheuints, addrs=None, sign: bool = False, first_bits=None):
        """addrs[i] <- Address::set_from_fheuint(fheuints[i]) (conversion.rs:68-82) for 1 to DERIVE_MAX encrypted integers as ONE launch
        on this Ram's stream (fheram_address_derive): no allocation, no host wait; later operations that use the addresses are ordered
        behind it.  addrs: existing Address objects to overwrite in place (from Address.alloc, host digits, encrypt_sk or an earlier
        derivation; no address twice), or None to allocate them.  sign=False: the convention Ram.read accepts.  Returns the addresses.
        first_bits: the address is read from bit first_bits[i] of integer i on (fheram_address_derive_at; a byte address keeps its lane
        offset in bits [0, 2) and its word address above them), one launch per distinct first bit."""
        return _derive_addresses(self, library().fheram_address_derive, fheuints, addrs, sign, first_bits, "fheram_address_derive_at")

    def write(self, w, address: Address, keys: EvaluationKeysPrepared):  # ram.rs:226
        self._use_keys(keys)
        if w is None:
            self._chk(library().fheram_write(self._h, None, self.params.word_size(), address._device(self)))
            return
        w = _i64(w)
        n_w = w.shape[0] if w.ndim > 1 else w.size // self.params.glwe_len()
        self._chk(library().fheram_write(self._h, _p(w), n_w, address._device(self)))

    # -- row-sharded path (every buffer: host int64 ndarray, or (device_ptr, True) for an int32 device buffer)
    @staticmethod
    def _buf(b):
        if isinstance(b, tuple):
            return C.c_void_p(int(b[0])), 1
        return b.ctypes.data_as(C.c_void_p), 0

    def read_partial(self, address: Address, keys: EvaluationKeysPrepared, prepare_write: bool = False, out=None):
        self._use_keys(keys)
        if out is None:
            out = self._out()
        ptr, dev = self._buf(out)
        self._chk(library().fheram_read_partial(self._h, address._device(self), int(prepare_write), ptr, dev))
        return out

    def read_finish(self, address: Address, keys: EvaluationKeysPrepared, partials, prepare_write: bool = False, download: bool = True):
        self._use_keys(keys)
        if not isinstance(partials, tuple):
            partials = _i64(partials)
        ptr, dev = self._buf(partials)
        out = self._out() if download else None
        self._chk(library().fheram_read_finish(self._h, address._device(self), int(prepare_write), ptr, dev, _p(out) if download else None))
        return out

    def write_root(self, w, address: Address, keys: EvaluationKeysPrepared, out=None):
        self._use_keys(keys)
        if out is None:
            out = self._out()
        ptr, dev = self._buf(out)
        wp = None if w is None else _p(_i64(w))
        self._chk(library().fheram_write_root(self._h, wp, self.params.word_size(), address._device(self), ptr, dev))
        return out

    def write_begin(self, address: Address, keys: EvaluationKeysPrepared):
        """start the part of a write that does not need ct_lo (overlaps the root's work and the broadcast)"""
        self._use_keys(keys)
        self._chk(library().fheram_write_begin(self._h, address._device(self)))

    def stream_signal(self, hip_stream: int):
        """work enqueued later on `hip_stream` (a hipStream_t as int, 0 = default stream) waits for this context"""
        self._chk(library().fheram_stream_signal(self._h, C.c_void_p(int(hip_stream))))

    def stream_wait(self, hip_stream: int):
        """work this context enqueues later waits for everything enqueued on `hip_stream` so far"""
        self._chk(library().fheram_stream_wait(self._h, C.c_void_p(int(hip_stream))))

    def device_malloc(self, n_bytes: int) -> int:
        """device memory on this context's GPU for exchange buffers (pass (ptr, True) to the sharded ops)"""
        out = C.c_void_p()
        self._chk(library().fheram_device_malloc(self._h, n_bytes, C.byref(out)))
        return int(out.value)

    def device_free(self, ptr: int):
        self._chk(library().fheram_device_free(self._h, C.c_void_p(int(ptr))))

    def write_shard(self, address: Address, keys: EvaluationKeysPrepared, ct_lo):
        self._use_keys(keys)
        if not isinstance(ct_lo, tuple):
            ct_lo = _i64(ct_lo)
        ptr, dev = self._buf(ct_lo)
        self._chk(library().fheram_write_shard(self._h, address._device(self), ptr, dev))

    def stage_words(self, w):
        w = _i64(w)
        self._chk(library().fheram_word_stage(self._h, _p(w), w.shape[0]))

    def result(self):
        out = self._out()
        self._chk(library().fheram_result_download(self._h, _p(out)))
        return out

    def result_view(self) -> np.ndarray:
        """the result of the last read in place (the context's pinned host buffer, fheram_result_map): valid until the
        next operation on this Ram — copy it if it has to live longer"""
        ptr = I64P()
        self._chk(library().fheram_result_map(self._h, C.byref(ptr)))
        p = self.params
        return np.ctypeslib.as_array(ptr, shape=(p.word_size(), p.glwe_len()))

    def sync(self):
        self._chk(library().fheram_sync(self._h))

    # -- the exactness contract of the FFT64 arithmetic, checked (fheram_roundoff_max)
    def roundoff_max(self, check: bool = True) -> float:
        """largest |x - rint(x)| any monitored rounding of an inverse transform has seen on this context since its creation / the
        last reset; raises FheRamError(8, PRECISION) above 3/8 unless check is False"""
        m = C.c_double()
        rc = library().fheram_roundoff_max(self._h, C.byref(m))
        if rc != 0 and (check or rc != 8):
            self._chk(rc)
        return float(m.value)

    def roundoff_reset(self):
        self._chk(library().fheram_roundoff_reset(self._h))

    # -- Poulpy-level ops (parity tests / micro-benchmarks)
    def glwe_external_product(self, a, ggsw):
        a = _i64(a).reshape(-1, self.params.glwe_len())
        res = np.zeros_like(a)
        self._chk(library().fheram_glwe_external_product(self._h, _p(a), a.shape[0], _p(_i64(ggsw).ravel()), _p(res)))
        return res

    def glwe_automorphism(self, keys, gal_el, mode, a):
        self._use_keys(keys)
        a = _i64(a).reshape(-1, self.params.glwe_len())
        res = np.zeros_like(a)
        self._chk(library().fheram_glwe_automorphism(self._h, mode, gal_el, _p(a), a.shape[0], _p(res)))
        return res

    def glwe_trace(self, keys, start, end, a):
        self._use_keys(keys)
        a = _i64(a).reshape(-1, self.params.glwe_len())
        res = np.zeros_like(a)
        self._chk(library().fheram_glwe_trace(self._h, start, end, _p(a), a.shape[0], _p(res)))
        return res

    def glwe_pack(self, keys, cts):
        self._use_keys(keys)
        cts = _i64(cts).reshape(-1, self.params.glwe_len())
        out = np.zeros(self.params.glwe_len(), dtype=np.int64)
        self._chk(library().fheram_glwe_pack(self._h, _p(cts), cts.shape[0], _p(out)))
        return out

    def ggsw_automorphism_inv(self, keys, ggsw):
        self._use_keys(keys)
        g = _i64(ggsw).ravel()
        out = np.zeros_like(g)
        self._chk(library().fheram_ggsw_automorphism_inv(self._h, _p(g), _p(out)))
        return out

    # -- measurement hooks
    def timer_begin(self):
        self._chk(library().fheram_timer_begin(self._h))

    def timer_end(self) -> float:
        ms = C.c_float()
        self._chk(library().fheram_timer_end(self._h, C.byref(ms)))
        return float(ms.value)

    def profile_enable(self, on=True):
        self._chk(library().fheram_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._chk(library().fheram_profile_reset(self._h))

    def profile_get(self, cls: str):
        a, b, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        self._chk(library().fheram_profile_get(self._h, cls.encode(), C.byref(a), C.byref(b), C.byref(ms)))
        return {"launches": int(a.value), "blocks": int(b.value), "ms": float(ms.value)}

    def tail_stats(self):
        """single-launch trace chains since the context was created, and how many of them fell back (fheram_tail_stats)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(library().fheram_tail_stats(self._h, C.byref(a), C.byref(b)))
        return {"launches": int(a.value), "fallbacks": int(b.value)}

    def mid_stats(self):
        """single-launch chains on 9..64 ciphertexts since the context was created, and how many ciphertexts were redone by the launch behind (fheram_mid_stats)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(library().fheram_mid_stats(self._h, C.byref(a), C.byref(b)))
        return {"launches": int(a.value), "fallbacks": int(b.value)}

    def mid_state(self):
        """setting of the single-launch mid chains in effect (0: switched off by the path itself) and how often it has been"""
        en, n = C.c_int(), C.c_uint64()
        self._chk(library().fheram_mid_state(self._h, C.byref(en), C.byref(n)))
        return {"enabled": int(en.value), "times_disabled": int(n.value)}

    def bench_external_product(self, batch: int, iters: int) -> float:
        """ms for a dependent chain of `iters` launches of `batch` GLWE x GGSW products (BASELINE.json configs[1])"""
        ms = C.c_float()
        self._chk(library().fheram_bench_external_product(self._h, batch, iters, C.byref(ms)))
        return float(ms.value)

    # -- self-test of the FP64 FFT arithmetic (tests/test_gpu_fft.py)
    def selftest_convolve(self, a, g, singles: bool = False):
        """raw (unrounded) sums  out[0] = sum_r a_r * g_r,  out[1] = sum_r a_r * g_{r ^ 1}  of negacyclic products of int32 polynomials"""
        a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1, self.params.n())
        g = np.ascontiguousarray(g, dtype=np.int32).reshape(-1, self.params.n())
        assert a.shape == g.shape
        out = np.zeros((2, self.params.n()), dtype=np.float64)
        ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
        self._chk(library().fheram_selftest_convolve(self._h, a.shape[0], ip(a), ip(g), out.ctypes.data_as(C.POINTER(C.c_double)), int(singles)))
        return out

    def selftest_convolve_rounded(self, a, g, operand_scale: float = 1.0):
        """the same sums ROUNDED as the path rounds them (through the round-off monitor); operand_scale = 0.5 drives the monitor over its limit"""
        a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1, self.params.n())
        g = np.ascontiguousarray(g, dtype=np.int32).reshape(-1, self.params.n())
        assert a.shape == g.shape
        out = np.zeros((2, self.params.n()), dtype=np.float64)
        ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
        self._chk(library().fheram_selftest_convolve_rounded(self._h, a.shape[0], ip(a), ip(g), out.ctypes.data_as(C.POINTER(C.c_double)), float(operand_scale)))
        return out

    # -- self-test of every transform form the kernels call (tests/test_gpu_fft_forms.py)
    SELFTEST_FORMS = ("skew<1,1>", "skew<2,1>", "skew<1,0> alternating", "skew<1,0> behind fwd", "skew<1,2>", "skew<2,2>",
                      "inv1_hooked<2>", "inv2_hooked<2>", "five-limb units")

    def selftest_forms(self, a, g, inv_form: int, fwd_polys: int = 2, rounded: bool = False, operand_scale: float = 1.0, spectra: bool = False):
        """a, g: [K][R][N] int32 -> out [K][2][N]: per batch the two sums of selftest_convolve, through ntt_fwd<fwd_polys> and inverse form
        `inv_form` (index into SELFTEST_FORMS), the batches one after the other in the same exchange buffers; raw doubles, or
        rounded through the round-off monitor.  spectra: also return the forward launch's scratch [2][K][R][N]."""
        n = self.params.n()
        a = np.ascontiguousarray(a, dtype=np.int32)
        g = np.ascontiguousarray(g, dtype=np.int32)
        assert a.ndim == 3 and a.shape == g.shape and a.shape[2] == n
        k, r = a.shape[0], a.shape[1]
        out = np.zeros((k, 2, n), dtype=np.float64)
        sp = np.zeros((2, k, r, n), dtype=np.float64) if spectra else None
        ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double)) if v is not None else None   # noqa: E731
        self._chk(library().fheram_selftest_forms(self._h, int(fwd_polys), int(inv_form), r, k, ip(a), ip(g), dp(out), int(bool(rounded)),
                                                  float(operand_scale), dp(sp)))
        return (out, sp) if spectra else out

    # -- self-test of the limb arithmetic (tests/test_gpu_limb_forms.py)
    LIMB_FORM_IN, LIMB_FORM_OUT = 10, 6

    def selftest_limb_forms(self, form: int, inputs):
        """one coefficient of limb form `form` (csrc/limb_forms_eval.hpp) per row of `inputs` [n][10] (exact integers as doubles): -> [n][6]"""
        inputs = np.ascontiguousarray(inputs, dtype=np.float64).reshape(-1, self.LIMB_FORM_IN)
        out = np.zeros((inputs.shape[0], self.LIMB_FORM_OUT), dtype=np.float64)
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        self._chk(library().fheram_selftest_limb_forms(self._h, int(form), inputs.shape[0], dp(inputs), dp(out)))
        return out

    def bench_chain(self, kind: int, batch: int, n: int, iters: int) -> float:
        """ms for `iters` back-to-back runs of a dependent chain on `batch` ciphertexts: kind 0 = n trace steps, 1 = n external products"""
        ms = C.c_float()
        self._chk(library().fheram_bench_chain(self._h, kind, batch, n, iters, C.byref(ms)))
        return float(ms.value)

    def device_info(self):
        buf = C.create_string_buffer(256)
        cus = C.c_int()
        self._chk(library().fheram_device_info(self._h, buf, 256, C.byref(cus)))
        return {"name": buf.value.decode(), "compute_units": int(cus.value)}


class GroupRam:
    """Ram (ram.rs:25-29) over several GPUs of one node behind ONE handle: the native row-sharded path (fheram_group_*,
    include/fheram.h) for a single-process host.  Same calls as Ram: read / read_prepare_write / write, one per op
    (ram.rs:172-176,196-200,226-231).  `devices`: HIP device indices, a power of two of them (the same index may repeat:
    rehearsal on one GPU)."""

    def __init__(self, params: Optional[Parameters], devices: Sequence[int]):
        self.params = params or Parameters.new()
        self.devices = [int(d) for d in devices]
        self._h = None
        L = library()
        out = C.c_void_p()
        cp = self.params._c()
        dv = (C.c_int * len(self.devices))(*self.devices)
        rc = L.fheram_group_create(C.byref(cp), dv, len(self.devices), C.byref(out))
        if rc != 0:
            raise FheRamError(rc, L.fheram_group_last_error(None).decode())
        self._h = out.value
        self._keys = None

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.fheram_group_destroy(self._h)
            self._h = None

    def _chk(self, rc):
        if rc != 0:
            raise FheRamError(rc, library().fheram_group_last_error(self._h).decode())

    def _use_keys(self, keys: EvaluationKeysPrepared):
        if self._keys is keys:
            return
        L = library()
        c0 = L.fheram_group_ctx(self._h, 0)
        atk_len, inv_len = L.fheram_atk_len(c0), L.fheram_evk_inv_len(c0)
        if keys.atk_glwe is None or any(k.size != atk_len for k in keys.atk_glwe) or keys.atk_ggsw_inv.size != inv_len or keys.tsk_ggsw_inv.size != inv_len:
            raise FheRamError(1, "evaluation-key layout does not match the group's (parameters.rs:71-93)")
        arr = (I64P * len(keys.atk_glwe))(*[_p(k) for k in keys.atk_glwe])
        self._chk(L.fheram_group_keys_load(self._h, _p(keys.gal_els), len(keys.gal_els), arr, _p(keys.atk_ggsw_inv),
                                           keys.atk_ggsw_inv_p, _p(keys.tsk_ggsw_inv)))
        self._keys = keys

    def _out(self):
        return np.zeros((self.params.word_size(), self.params.glwe_len()), dtype=np.int64)

    def load_encrypted(self, rows: np.ndarray):
        """rows: the whole RAM, [word_size][rows][GLWE] (Ram::encrypt_sk output, ram.rs:129-167)"""
        p = self.params
        rows = _i64(rows)
        if rows.size != p.word_size() * p.rows() * p.glwe_len():
            raise FheRamError(1, f"invalid data: expected {p.word_size()}x{p.rows()} GLWE rows (ram.rs:144-155)")
        self._chk(library().fheram_group_ram_upload(self._h, _p(rows)))

    def store_encrypted(self) -> np.ndarray:
        p = self.params
        rows = np.zeros((p.word_size(), p.rows(), p.glwe_len()), dtype=np.int64)
        self._chk(library().fheram_group_ram_download(self._h, _p(rows)))
        return rows

    def tree(self, level: int = 0) -> np.ndarray:
        out = self._out()
        self._chk(library().fheram_group_ram_tree_download(self._h, level, _p(out)))
        return out

    @property
    def state(self) -> bool:
        return bool(library().fheram_group_ram_state(self._h))

    def read(self, address: Address, keys: EvaluationKeysPrepared, download: bool = True):  # ram.rs:172
        self._use_keys(keys)
        out = self._out() if download else None
        self._chk(library().fheram_group_read(self._h, address._group(self), _p(out) if download else None))
        return out

    def read_prepare_write(self, address: Address, keys: EvaluationKeysPrepared, download: bool = True):  # ram.rs:196
        self._use_keys(keys)
        out = self._out() if download else None
        self._chk(library().fheram_group_read_prepare_write(self._h, address._group(self), _p(out) if download else None))
        return out

    def write(self, w, address: Address, keys: EvaluationKeysPrepared):  # ram.rs:226
        self._use_keys(keys)
        ws = self.params.word_size()
        if w is None:
            self._chk(library().fheram_group_write(self._h, None, ws, address._group(self)))
            return
        w = _i64(w)
        n_w = w.shape[0] if w.ndim > 1 else w.size // self.params.glwe_len()
        self._chk(library().fheram_group_write(self._h, _p(w), n_w, address._group(self)))

    def stage_words(self, w):
        w = _i64(w)
        self._chk(library().fheram_group_word_stage(self._h, _p(w), w.shape[0]))

    def result(self):
        out = self._out()
        self._chk(library().fheram_group_result_download(self._h, _p(out)))
        return out

    def peer_info(self) -> List[bool]:
        """per shard: the exchange copies between its device and the root's go peer to peer (the self-test copies of the
        constructor went through either way)"""
        n = len(self.devices)
        d = (C.c_int * n)()
        self._chk(library().fheram_group_peer_info(self._h, d, n))
        return [bool(x) for x in d]

    @property
    def poisoned(self) -> bool:
        """an op failed part-way: every further op is refused until load_encrypted has replaced the rows"""
        return bool(library().fheram_group_poisoned(self._h))

    def roundoff_max(self) -> float:
        """the largest round-off over the shards' monitors (fheram_group_roundoff_max); raises PRECISION above 3/8"""
        m = C.c_double()
        self._chk(library().fheram_group_roundoff_max(self._h, C.byref(m)))
        return float(m.value)


class RamBank:
    """M RAMs of the same shape under ONE prepared key set on one GPU (fheram_bank): read / read_prepare_write / write on a
    contiguous member range [first, first + len(addresses)) as ONE operation, one address per member.  Member m behaves exactly like a
    standalone Ram driven through the same calls (int64-identical results, rows, tree and state); members outside a range are
    untouched, and a refused call changes no member."""

    def __init__(self, params: Optional[Parameters], n_members: int, device: int = 0, config: Optional[dict] = None):
        """config: execution switches that differ from fheram_config_default(), as Ram's"""
        self.params = params or Parameters.new()
        self.n_members = int(n_members)
        self._h = None
        L = library()
        out = C.c_void_p()
        cp = self.params._c()
        cfg = _c_config(config)
        rc = L.fheram_bank_create(C.byref(cp), device, self.n_members, C.byref(cfg) if cfg is not None else None, C.byref(out))
        if rc != 0:
            raise FheRamError(rc, L.fheram_bank_last_error(None).decode())
        self._h = out.value
        self._keys = None

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.fheram_bank_destroy(self._h)
            self._h = None

    def __len__(self):
        return library().fheram_bank_size(self._h)

    def _chk(self, rc):
        if rc != 0:
            raise FheRamError(rc, library().fheram_bank_last_error(self._h).decode())

    def _use_keys(self, keys: EvaluationKeysPrepared):
        if self._keys is keys:
            return
        if keys.atk_glwe is None:
            raise FheRamError(5, "these keys were generated on another context's device (EvaluationKeysPrepared.encrypt_sk "
                                 "without keep_std=True): their std forms are not on the host")
        p = self.params
        n, b2k = p.n(), p.basek()
        atk_len = p.dnum_ct() * -(-p.k_evk_trace() // b2k) * 2 * n        # evk_glwe_infos, parameters.rs:71-81
        inv_len = p.dnum_ggsw() * -(-p.k_evk_ggsw_inv() // b2k) * 2 * n   # evk_ggsw_infos, parameters.rs:83-93
        if any(k.size != atk_len for k in keys.atk_glwe) or keys.atk_ggsw_inv.size != inv_len or keys.tsk_ggsw_inv.size != inv_len:
            raise FheRamError(1, f"evaluation-key layout does not match the bank's (trace keys of {atk_len} limbs-elements, "
                                 f"inverse / tensor keys of {inv_len}: evk_glwe_infos / evk_ggsw_infos, parameters.rs:71-93)")
        arr = (I64P * len(keys.atk_glwe))(*[_p(k) for k in keys.atk_glwe])
        self._chk(library().fheram_bank_keys_load(self._h, _p(keys.gal_els), len(keys.gal_els), arr, _p(keys.atk_ggsw_inv),
                                                  keys.atk_ggsw_inv_p, _p(keys.tsk_ggsw_inv)))
        self._keys = keys

    def _member(self, member: int) -> int:
        member = int(member)
        if not 0 <= member < self.n_members:
            raise FheRamError(1, f"member {member} is outside the bank's {self.n_members} members")
        return member

    def _range(self, first: int, n: int):
        first, n = int(first), int(n)
        if n < 1 or first < 0 or first + n > self.n_members:
            raise FheRamError(1, f"member range [{first}, {first + n}) is empty or outside the bank's {self.n_members} members")
        return first, n

    # -- data hand-over
    def load_encrypted(self, member: int, rows: np.ndarray):
        """rows: [word_size][rows][GLWE] of one member, which becomes readable"""
        p = self.params
        rows = _i64(rows)
        if rows.size != p.word_size() * p.rows() * p.glwe_len():
            raise FheRamError(1, f"invalid data: expected {p.word_size()}x{p.rows()} GLWE rows (ram.rs:144-155)")
        self._chk(library().fheram_bank_ram_upload(self._h, self._member(member), _p(rows)))

    def store_encrypted(self, member: int) -> np.ndarray:
        p = self.params
        rows = np.zeros((p.word_size(), p.rows(), p.glwe_len()), dtype=np.int64)
        self._chk(library().fheram_bank_ram_download(self._h, self._member(member), _p(rows)))
        return rows

    def tree(self, member: int, level: int = 0) -> np.ndarray:
        out = np.zeros((self.params.word_size(), self.params.glwe_len()), dtype=np.int64)
        self._chk(library().fheram_bank_ram_tree_download(self._h, self._member(member), level, _p(out)))
        return out

    def state(self, member: int) -> bool:
        return bool(library().fheram_bank_ram_state(self._h, self._member(member)))

    # -- the path
    def _addrs(self, addresses, first):
        addresses = list(addresses)
        if not all(isinstance(a, Address) for a in addresses):
            raise FheRamError(1, "every entry must be an Address (a null address is refused)")
        first, n = self._range(first, len(addresses))
        return first, n, (C.c_void_p * n)(*[a._bank(self) for a in addresses])

    def _read(self, fn, addresses, keys, first, download):
        first, n, arr = self._addrs(addresses, first)
        self._use_keys(keys)
        p = self.params
        out = np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64) if download else None
        self._chk(fn(self._h, first, n, arr, _p(out) if download else None))
        return out

    def read(self, addresses, keys: EvaluationKeysPrepared, first: int = 0, download: bool = True):  # ram.rs:172, per member
        """members first .. first + len(addresses) - 1 read at one address each: int64 [n][word_size][GLWE]"""
        return self._read(library().fheram_bank_read, addresses, keys, first, download)

    def read_prepare_write(self, addresses, keys: EvaluationKeysPrepared, first: int = 0, download: bool = True):  # ram.rs:196
        return self._read(library().fheram_bank_read_prepare_write, addresses, keys, first, download)

    def write(self, words, addresses, keys: EvaluationKeysPrepared, first: int = 0):  # ram.rs:226, per member
        """words: [n][word_size][GLWE], member first + k's word at k"""
        first, n, arr = self._addrs(addresses, first)
        p = self.params
        if words is None:
            raise FheRamError(1, "null words")
        w = _i64(words)
        if w.size != n * p.word_size() * p.glwe_len():
            raise FheRamError(1, f"w.len() != subrams.len() (ram.rs:243): expected {n} x {p.word_size()} GLWEs")
        self._use_keys(keys)
        self._chk(library().fheram_bank_write(self._h, first, n, _p(w), arr))

    def read_list(self, members, addresses, keys: EvaluationKeysPrepared, download: bool = True):
        """K reads as ONE operation (fheram_bank_read_list), entry k on member members[k] at addresses[k]: any order, any repetition,
        any subset of the members; 1 <= K <= READ_LIST_MAX and K * word_size <= 64.  int64 [K][word_size][GLWE], slice k equal to
        read([addresses[k]], keys, first=members[k]); the bank is left where that sequence of single-member reads leaves it, and
        members that are not named are untouched.  download=False: no host wait (list_result later)."""
        members, addresses = [int(m) for m in members], list(addresses)
        if not 1 <= len(members) <= READ_LIST_MAX or len(addresses) != len(members):
            raise FheRamError(1, f"read_list takes 1 to {READ_LIST_MAX} members and as many addresses, got {len(members)} and {len(addresses)}")
        if not all(isinstance(a, Address) for a in addresses):
            raise FheRamError(1, "every entry must be an Address (a null address is refused)")
        n = len(members)
        for m in members:
            self._member(m)
        arr = (C.c_void_p * n)(*[a._bank(self) for a in addresses])
        self._use_keys(keys)
        p = self.params
        out = np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64) if download else None
        self._chk(library().fheram_bank_read_list(self._h, (C.c_int * n)(*members), arr, n, _p(out) if download else None))
        return out

    def list_result(self, first: int = 0, n: int = 1) -> np.ndarray:
        """entries [first, first + n) of the last read_list: int64 [n][word_size][GLWE]"""
        first, n = int(first), int(n)
        p = self.params
        out = np.zeros((max(n, 1), p.word_size(), p.glwe_len()), dtype=np.int64)
        self._chk(library().fheram_bank_read_list_result(self._h, first, n, _p(out)))
        return out

    def _list_args(self, what, members, addresses):
        members, addresses = [int(m) for m in members], list(addresses)
        if not members or len(addresses) != len(members):
            raise FheRamError(1, f"{what} takes at least one member and as many addresses, got {len(members)} and {len(addresses)}")
        if not all(isinstance(a, Address) for a in addresses):
            raise FheRamError(1, "every entry must be an Address (a null address is refused)")
        n = len(members)
        return n, (C.c_int * n)(*members), (C.c_void_p * n)(*[a._bank(self) for a in addresses])

    def read_prepare_write_list(self, members, addresses, keys: EvaluationKeysPrepared, download: bool = True):
        """read_prepare_write of ANY set of members as ONE operation (fheram_bank_read_prepare_write_list), entry k on member members[k] at
        addresses[k]: distinct members, any order, any subset (a RAM has one pending write, so a member named twice is refused).  int64
        [n][word_size][GLWE], slice k equal to read_prepare_write([addresses[k]], keys, first=members[k]); every named member is then
        prepared like any other (write_list, write on a range and result all work on it), members that are not named are untouched.
        download=False: no host wait (result(first=m, n=1) later)."""
        n, mem, arr = self._list_args("read_prepare_write_list", members, addresses)
        self._use_keys(keys)
        p = self.params
        out = np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64) if download else None
        self._chk(library().fheram_bank_read_prepare_write_list(self._h, mem, arr, n, _p(out) if download else None))
        return out

    def write_list(self, members, words, addresses, keys: EvaluationKeysPrepared):
        """write of ANY set of prepared members as ONE operation (fheram_bank_write_list): words [n][word_size][GLWE], entry k to member
        members[k] at addresses[k]; the members may have been prepared by a list, a range or single calls.  Never waits for the device."""
        n, mem, arr = self._list_args("write_list", members, addresses)
        p = self.params
        if words is None:
            raise FheRamError(1, "null words")
        w = _i64(words)
        if w.size != n * p.word_size() * p.glwe_len():
            raise FheRamError(1, f"w.len() != subrams.len() (ram.rs:243): expected {n} x {p.word_size()} GLWEs")
        self._use_keys(keys)
        self._chk(library().fheram_bank_write_list(self._h, mem, arr, n, _p(w)))

    def selftest_fail_list_alloc(self, nth: int):
        """self-test: the nth device allocation the write lists' buffers ask for from now on fails once (0: none)"""
        self._chk(library().fheram_bank_selftest_fail_list_alloc(self._h, int(nth)))

    def derive_addresses(self, fheuints, addrs=None, sign: bool = False, first_bits=None):
        """as Ram.derive_addresses, with integers and addresses bound to this bank (FheUintPrepared.from_host(bank, ...),
        Address.alloc(bank)): a derived address is an ordinary bank address and may serve several members"""
        return _derive_addresses(self, library().fheram_bank_address_derive, fheuints, addrs, sign, first_bits, "fheram_bank_address_derive_at")

    def derive_list(self, items):
        """any mix of addresses, selectors and selector fields from encrypted integers as ONE launch (fheram_bank_derive_list): `items` are
        Derive entries (the lists Derive.fields returns are flattened).  No host wait, in place; returns the targets in item order.  An
        address item with addr=None gets an Address.alloc(bank): that allocation is this mirror's convenience, made after its own checks
        and before the library call (which allocates nothing), and freed again if the library refuses the call."""
        flat = []
        for it in items:
            flat.extend(it if isinstance(it, (list, tuple)) else [it])
        if not all(isinstance(it, Derive) for it in flat):
            raise FheRamError(1, "derive_list takes Derive entries (Derive.address, Derive.selector, Derive.fields)")
        n = len(flat)
        if not 1 <= n <= DERIVE_LIST_MAX:
            raise FheRamError(1, f"derive_list takes 1 to DERIVE_LIST_MAX = {DERIVE_LIST_MAX} items, got {n}")
        targets = [Address.alloc(self) if it.kind == DERIVE_ADDRESS and it.target is None else it.target for it in flat]
        arr = (_CDeriveItem * n)()
        for i, (it, t) in enumerate(zip(flat, targets)):
            handle = t._bank(self) if it.kind == DERIVE_ADDRESS else t._h   # (an address made from host digits: created here)
            arr[i] = _CDeriveItem(it.kind, it.first_bit, int(it.sign), it.field, it.fu._h, handle)
        try:
            self._chk(library().fheram_bank_derive_list(self._h, arr, n))
        except FheRamError:
            for it, t in zip(flat, targets):
                if it.target is None:
                    t._handles.clear()   # the addresses allocated above go with the refusal (their handles free the device buffers)
            raise
        fed = {}
        for it, t in zip(flat, targets):
            if it.kind == DERIVE_ADDRESS:
                t._digits = None                                   # the host copy, and the handles on other devices, held the old digits
                t._handles = {id(self): t._handles[id(self)]}
            fed.setdefault(id(t), (t, []))[1].append(it.fu)
        for t, fus in fed.values():
            t._derived_from = fus if len(fus) > 1 else fus[0]      # the integers stay alive until the launch that reads them has run
        return targets

    def address_digits(self, addr: Address) -> np.ndarray:
        """the std-form GGSW digits of a bank address, [n_digits][ggsw_len] (fheram_bank_address_download)"""
        if not isinstance(addr, Address):
            raise FheRamError(1, "address_digits takes an Address")
        out = np.zeros((addr.base2d.as_1d().size(), self.params.ggsw_len()), dtype=np.int64)
        self._chk(library().fheram_bank_address_download(self._h, addr._bank(self), _p(out)))
        return out

    # -- oblivious select (include/fheram.h: pick a word by an encrypted index)
    def selector(self, bits: int) -> Selector:
        """a selector of `bits` bits with its buffers and no digits yet (fheram_bank_selector_alloc): what derive_selectors fills"""
        out = C.c_void_p()
        self._chk(library().fheram_bank_selector_alloc(self._h, int(bits), C.byref(out)))
        return Selector(self, out.value, bits)

    def derive_selectors(self, fheuints, first_bits, sels):
        """sels[i] <- bits [first_bits[i], first_bits[i] + sels[i].bits) of fheuints[i] (fheram_bank_selector_derive): one launch per
        distinct (first_bit, bits) pair, no allocation, no host wait, in place"""
        fheuints, first_bits, sels = list(fheuints), [int(f) for f in first_bits], list(sels)
        k = len(sels)
        if not 1 <= k <= SELECT_MAX or len(fheuints) != k or len(first_bits) != k:
            raise FheRamError(1, f"derive_selectors takes 1 to SELECT_MAX = {SELECT_MAX} selectors and as many integers and first bits")
        if not all(isinstance(f, FheUintPrepared) for f in fheuints) or not all(isinstance(s, Selector) for s in sels):
            raise FheRamError(1, "derive_selectors: every integer must be a FheUintPrepared and every selector a Selector")
        fa, sa = (C.c_void_p * k)(*[f._h for f in fheuints]), (C.c_void_p * k)(*[s._h for s in sels])
        self._chk(library().fheram_bank_selector_derive(self._h, fa, (C.c_int * k)(*first_bits), k, sa))
        for s, f in zip(sels, fheuints):
            s._derived_from = f   # the integer stays alive until the launch that reads it has run
        return sels

    def selector_fields(self, widths) -> Selector:
        """a field selector with its buffers and no digits yet (fheram_bank_selector_alloc_fields): digit d has widths[d] bits at bit offset
        sum(widths[:d]); derive_selector_fields fills it"""
        widths = [int(x) for x in widths]
        out = C.c_void_p()
        self._chk(library().fheram_bank_selector_alloc_fields(self._h, (C.c_int * max(len(widths), 1))(*widths), len(widths), C.byref(out)))
        s = Selector(self, out.value, sum(widths))
        s.widths = widths
        return s

    def derive_selector_fields(self, sel, fheuints, first_bits):
        """digit d of the field selector `sel` <- bits [first_bits[d], first_bits[d] + widths[d]) of fheuints[d]
        (fheram_bank_selector_derive_fields): one launch per field, no allocation, no host wait, in place"""
        fheuints, first_bits = list(fheuints), [int(f) for f in first_bits]
        if not isinstance(sel, Selector) or sel.widths is None:
            raise FheRamError(1, "derive_selector_fields takes a field selector (RamBank.selector_fields, Selector.from_digits_fields)")
        k = len(sel.widths)
        if len(fheuints) != k or len(first_bits) != k or not all(isinstance(f, FheUintPrepared) for f in fheuints):
            raise FheRamError(1, f"derive_selector_fields: a selector of {k} fields takes {k} FheUintPrepared and {k} first bits")
        self._chk(library().fheram_bank_selector_derive_fields(self._h, sel._h, (C.c_void_p * k)(*[f._h for f in fheuints]), (C.c_int * k)(*first_bits)))
        sel._derived_from = fheuints   # the integers stay alive until the launches that read them have run
        return sel

    def select_lanes(self, sels, candidates, host_words=None, download: bool = True, keys: Optional[EvaluationKeysPrepared] = None):
        """n selects as ONE operation with lane-mapped candidates (fheram_bank_select_lanes): candidates[k][j] is a list of word_size Lane,
        the byte ciphertexts candidate j of select k is assembled from (store_merge_lanes / load_extract_lanes build such lists).
        Everything else is select's: host_words, download, keys, and it is the last select for select_result / write_list_selected."""
        sels, candidates = list(sels), [[list(c) for c in cs] for cs in candidates]
        n = len(sels)
        if n < 1 or len(candidates) != n or not all(isinstance(s, Selector) for s in sels):
            raise FheRamError(1, "select_lanes takes at least one Selector and one candidate list per selector")
        p = self.params
        ws = p.word_size()
        words = [c for cs in candidates for c in cs]
        if not words or not all(len(c) == ws and all(isinstance(l, Lane) for l in c) for c in words):
            raise FheRamError(1, f"every candidate must be a list of word_size = {ws} Lane")
        flat = [l for c in words for l in c]
        per = ws * p.glwe_len()
        hw = None
        if host_words is not None:
            hw = _i64(host_words)
            slots = [l.index for l in flat if l.kind == SRC_HOST]
            if slots and (min(slots) < 0 or (max(slots) + 1) * per > hw.size):
                raise FheRamError(1, f"a host lane names a slot outside host_words ({hw.size // per} slots of {ws} GLWEs)")
        lanes = (_CSelectLane * len(flat))(*[_CSelectLane(l.kind, l.index, l.lane, l.reserved) for l in flat])
        if keys is not None:
            self._use_keys(keys)
        out = np.zeros((n, ws, p.glwe_len()), dtype=np.int64) if download else None
        self._chk(library().fheram_bank_select_lanes(self._h, (C.c_void_p * n)(*[s._h for s in sels]), (C.c_int * n)(*[len(c) for c in candidates]), n,
                                                     lanes, _p(hw) if hw is not None else None, _p(out) if download else None))
        return out

    def select(self, sels, candidates, host_words=None, download: bool = True, keys: Optional[EvaluationKeysPrepared] = None):
        """n selects as ONE operation (fheram_bank_select): candidates[k] is the list of Src of select k, of which sels[k] picks one.
        host_words: [..][word_size][GLWE], the slots Src.host(i) names.  int64 [n][word_size][GLWE]; download=False: no host wait
        (select_result later).  keys: loaded first when given (else the bank's loaded keys).  No member, and no result of an earlier
        read list, is touched."""
        sels, candidates = list(sels), [list(c) for c in candidates]
        n = len(sels)
        if n < 1 or len(candidates) != n or not all(isinstance(s, Selector) for s in sels):
            raise FheRamError(1, "select takes at least one Selector and one candidate list per selector")
        flat = [s for c in candidates for s in c]
        if not flat or not all(isinstance(s, Src) for s in flat):
            raise FheRamError(1, "every candidate must be a Src")
        p = self.params
        per = p.word_size() * p.glwe_len()
        hw = None
        if host_words is not None:
            hw = _i64(host_words)
            slots = [s.index for s in flat if s.kind == SRC_HOST]
            if slots and (min(slots) < 0 or (max(slots) + 1) * per > hw.size):
                raise FheRamError(1, f"a host candidate names a slot outside host_words ({hw.size // per} slots of {p.word_size()} GLWEs)")
        srcs = (_CSelectSrc * len(flat))(*[_CSelectSrc(s.kind, s.index) for s in flat])
        if keys is not None:
            self._use_keys(keys)
        out = np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64) if download else None
        self._chk(library().fheram_bank_select(self._h, (C.c_void_p * n)(*[s._h for s in sels]), (C.c_int * n)(*[len(c) for c in candidates]), n,
                                               srcs, _p(hw) if hw is not None else None, _p(out) if download else None))
        return out

    def select_result(self, first: int = 0, n: int = 1) -> np.ndarray:
        """outputs [first, first + n) of the last select: int64 [n][word_size][GLWE]"""
        first, n = int(first), int(n)
        p = self.params
        out = np.zeros((max(n, 1), p.word_size(), p.glwe_len()), dtype=np.int64)
        self._chk(library().fheram_bank_select_result(self._h, first, n, _p(out)))
        return out

    def write_list_selected(self, members, picks, addresses, keys: EvaluationKeysPrepared):
        """write_list whose words are outputs of the last select (fheram_bank_write_list_selected): entry k writes output picks[k] to
        member members[k] at addresses[k]; the words never leave the device.  Never waits for the device."""
        n, mem, arr = self._list_args("write_list_selected", members, addresses)
        picks = [int(x) for x in picks]
        if len(picks) != n:
            raise FheRamError(1, f"write_list_selected: {n} members need {n} picks")
        self._use_keys(keys)
        self._chk(library().fheram_bank_write_list_selected(self._h, mem, arr, n, (C.c_int * n)(*picks)))

    # -- register files (include/fheram.h: a one-row RAM read and written by selectors)
    def regfile(self, bits: int) -> RegFile:
        """a register file of 2^bits words with every device buffer it will need (fheram_bank_regs_create); RegFile.load / pack fill it"""
        out = C.c_void_p()
        self._chk(library().fheram_bank_regs_create(self._h, int(bits), C.byref(out)))
        return RegFile(self, out.value, bits)

    def scratch(self, bits: int) -> RegFile:
        """a WIDE register file of 2^bits words, 1 <= bits <= TABLE_BITS_MAX (fheram_bank_regs_create_wide): a writable one-row memory of
        up to 4096 words.  Above SELECT_BITS_MAX bits its addresses are wide Selectors (table_selector / table_selector_fields)."""
        bits = int(bits)
        if not 1 <= bits <= TABLE_BITS_MAX:
            raise FheRamError(1, f"bits = {bits} is outside [1, TABLE_BITS_MAX = {TABLE_BITS_MAX}]")
        out = C.c_void_p()
        self._chk(library().fheram_bank_regs_create_wide(self._h, bits, C.byref(out)))
        return RegFile(self, out.value, bits)

    # -- tables (include/fheram.h: read-only one-row RAMs of up to 4096 words, read by wide selectors)
    def table(self, bits: int) -> Table:
        """a table of 2^bits words, bits <= TABLE_BITS_MAX, with every device buffer it will need (fheram_bank_table_create); Table.load /
        load_plain fill it"""
        out = C.c_void_p()
        self._chk(library().fheram_bank_table_create(self._h, int(bits), C.byref(out)))
        return Table(self, out.value, bits)

    def table_selector(self, bits: int, ggsw_digits=None) -> Selector:
        """a WIDE selector of up to TABLE_BITS_MAX bits: without digits (fheram_bank_table_selector_alloc; derive_selectors / derive_list
        fill it), or from host std-form GGSW digits (fheram_bank_table_selector_create).  It addresses a Table or a wide RegFile
        (scratch) of its bits; select refuses it above SELECT_BITS_MAX bits."""
        out = C.c_void_p()
        if ggsw_digits is None:
            self._chk(library().fheram_bank_table_selector_alloc(self._h, int(bits), C.byref(out)))
        else:
            digits = [_i64(g).ravel() for g in ggsw_digits]
            arr = (I64P * max(len(digits), 1))(*[_p(d) for d in digits])
            self._chk(library().fheram_bank_table_selector_create(self._h, arr, len(digits), int(bits), C.byref(out)))
        return Selector(self, out.value, bits)

    def table_selector_fields(self, widths) -> Selector:
        """a wide FIELD selector without digits (fheram_bank_table_selector_alloc_fields): up to SELECTOR_WIDE_DIGITS_MAX fields whose
        widths sum to at most TABLE_BITS_MAX; derive_selector_fields / Derive.fields fill it"""
        widths = [int(x) for x in widths]
        out = C.c_void_p()
        self._chk(library().fheram_bank_table_selector_alloc_fields(self._h, (C.c_int * max(len(widths), 1))(*widths), len(widths), C.byref(out)))
        s = Selector(self, out.value, sum(widths))
        s.widths = widths
        return s

    def table_read(self, tables, sels, download: bool = True, keys: Optional[EvaluationKeysPrepared] = None):
        """len(sels) reads as ONE operation (fheram_bank_table_read): entry k reads tables[k] at sels[k]; the same Table may appear several
        times and several Tables may share a call.  int64 [n][word_size][GLWE]; download=False: no host wait (table_result later)"""
        tables, sels = list(tables), list(sels)
        n = len(sels)
        if n < 1 or len(tables) != n:
            raise FheRamError(1, "table_read takes at least one Selector and one Table per selector")
        if not all(isinstance(t, Table) for t in tables) or not all(isinstance(s, Selector) for s in sels):
            raise FheRamError(1, "table_read takes Tables and Selectors")
        if keys is not None:
            self._use_keys(keys)
        p = self.params
        out = np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64) if download else None
        self._chk(library().fheram_bank_table_read(self._h, (C.c_void_p * n)(*[t._h for t in tables]), (C.c_void_p * n)(*[s._h for s in sels]), n,
                                                   _p(out) if download else None))
        return out

    def table_result(self, first: int = 0, n: int = 1) -> np.ndarray:
        """outputs [first, first + n) of the bank's last table read (fheram_bank_table_result)"""
        first, n = int(first), int(n)
        p = self.params
        out = np.zeros((max(n, 1), p.word_size(), p.glwe_len()), dtype=np.int64)
        self._chk(library().fheram_bank_table_result(self._h, first, n, _p(out)))
        return out

    # -- the public side (include/fheram.h): plain image loads, peek and poke at public addresses
    def load_plain(self, member: int, data, first_row: int = 0):
        """public bytes into the rows of one member from first_row on, as the trivial ciphertexts (fheram_bank_ram_load_plain): no host
        encryption, no keys, no secret.  data: whole words in Ram::encrypt_sk's layout (byte w of word j at data[j * word_size + w]),
        word 0 of data at address first_row * N; it covers whole rows, or ends where the member does.  first_row = 0 with
        max_addr * word_size bytes loads the whole member, which becomes readable as after load_encrypted."""
        p = self.params
        member = self._member(member)
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).ravel())
        first_row, ws, n = int(first_row), p.word_size(), p.n()
        if not 0 <= first_row < p.rows():
            raise FheRamError(1, f"row {first_row} is outside the member's {p.rows()} rows")
        if data.size == 0 or data.size % ws:
            raise FheRamError(1, f"invalid data: {data.size} bytes are not a positive number of words of word_size = {ws} bytes")
        words = data.size // ws
        last = first_row * n + words
        if last > p.max_addr() or (last % n and last != p.max_addr()):
            raise FheRamError(1, f"invalid data: {words} words from row {first_row} on neither fill whole rows nor end at max_addr = {p.max_addr()}")
        n_rows = -(-words // n)
        self._chk(library().fheram_bank_ram_load_plain(self._h, member, first_row, n_rows, data.ctypes.data_as(C.POINTER(C.c_uint8)), data.size))

    def _public_entries(self, what, members, addresses):
        members, addresses = [int(m) for m in members], [int(a) for a in addresses]
        n = len(members)
        if not 1 <= n <= PEEK_MAX or len(addresses) != n:
            raise FheRamError(1, f"{what} takes 1 to PEEK_MAX = {PEEK_MAX} members and as many addresses, got {len(members)} and {len(addresses)}")
        if n * self.params.word_size() > 64:
            raise FheRamError(1, f"{what}: n * word_size = {n * self.params.word_size()} exceeds 64")
        for m in members:
            self._member(m)
        for a in addresses:
            if not 0 <= a < self.params.max_addr():
                raise FheRamError(1, f"{what}: address {a} is outside max_addr = {self.params.max_addr()}")
        return n, (C.c_int * n)(*members), (C.c_uint64 * n)(*addresses)

    def peek(self, members, addresses, download: bool = True, keys: Optional[EvaluationKeysPrepared] = None):
        """len(members) reads at PUBLIC word addresses as ONE operation (fheram_bank_peek): entry k reads member members[k] at
        addresses[k]; members and addresses may repeat.  int64 [n][word_size][GLWE], each an encryption of [v, 0, .., 0]; download=False:
        no host wait (peek_result later).  Nothing of the bank changes but the last peek (Src.peek(k))."""
        n, mem, adr = self._public_entries("peek", members, addresses)
        if keys is not None:
            self._use_keys(keys)
        p = self.params
        out = np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64) if download else None
        self._chk(library().fheram_bank_peek(self._h, mem, adr, n, _p(out) if download else None))
        return out

    def peek_result(self, first: int = 0, n: int = 1) -> np.ndarray:
        """outputs [first, first + n) of the bank's last peek, or the old words of its last poke (fheram_bank_peek_result)"""
        first, n = int(first), int(n)
        p = self.params
        out = np.zeros((max(n, 1), p.word_size(), p.glwe_len()), dtype=np.int64)
        self._chk(library().fheram_bank_peek_result(self._h, first, n, _p(out)))
        return out

    def poke(self, members, addresses, words=None, srcs=None, keys: Optional[EvaluationKeysPrepared] = None):
        """len(members) writes at PUBLIC word addresses as ONE operation (fheram_bank_poke): entry k writes at addresses[k] of member
        members[k]; the (member, address) pairs are distinct.  Either words: int64 [n][word_size][GLWE] host ciphertexts, entry k's at
        k — or srcs: one Src per entry, with words the host_words its Src.host(i) name.  Every entry sees the rows as they were
        before the call; the OLD words are the last peek afterwards (peek_result, Src.peek(k)).  Never waits for the device."""
        n, mem, adr = self._public_entries("poke", members, addresses)
        if len(set(zip(mem, adr))) != n:
            raise FheRamError(1, "the targets of a poke are distinct (member, address) pairs")
        if srcs is None:
            if words is None:
                raise FheRamError(1, "poke takes words, or srcs")
            srcs = [Src.host(k) for k in range(n)]
            if _i64(words).size != n * self.params.word_size() * self.params.glwe_len():
                raise FheRamError(1, f"poke: expected {n} x {self.params.word_size()} GLWEs of words")
        srcs = list(srcs)
        if len(srcs) != n or not all(isinstance(s, Src) for s in srcs):
            raise FheRamError(1, f"poke takes one Src per entry, got {len(srcs)} for {n} entries")
        slots = [s.index for s in srcs if s.kind == SRC_HOST]
        if slots and words is None:
            raise FheRamError(1, "a host source needs words")
        if slots and max(slots) >= PEEK_MAX:
            raise FheRamError(1, f"a poke takes host slots [0, PEEK_MAX = {PEEK_MAX})")
        hw = self._host_words(words, slots)
        if keys is not None:
            self._use_keys(keys)
        arr = (_CSelectSrc * n)(*[_CSelectSrc(s.kind, s.index) for s in srcs])
        self._chk(library().fheram_bank_poke(self._h, mem, adr, n, arr, _p(hw) if hw is not None else None))

    def selftest_fail_public_alloc(self, nth: int):
        """self-test: the nth device allocation the public side's buffers ask for from now on fails once (0: none)"""
        self._chk(library().fheram_bank_selftest_fail_public_alloc(self._h, int(nth)))

    def read_mix(self, list=None, tables=None, regs=None, download: bool = True, keys: Optional[EvaluationKeysPrepared] = None):
        """a read list, a table read and a register read as ONE operation with one top (fheram_bank_read_mix).
        list = (members, addresses), tables = (tables, selectors), regs = (regfile, selectors); a group may be left out (None, or empty
        lists) but not all three, and the groups hold at most MIX_MAX entries together.  Entry k of a group equals output k of
        read_list / table_read / RegFile.read, and the bank is left where that sequence leaves it (list_result, table_result and
        RegFile.result read the groups' outputs; a group left out keeps its kind's last outputs).  Returns (list, table, regs): int64
        [n][word_size][GLWE] per group, None for a group left out; download=False: no host wait, (None, None, None)."""
        cm, keep, counts = RamBank._mix_reads(self, "read_mix", list, tables, regs, 0)
        if sum(counts) < 1:
            raise FheRamError(1, "read_mix takes at least one read: all three groups are empty")
        if keys is not None:
            self._use_keys(keys)
        p = self.params
        outs = [np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64) if (download and n) else None for n in counts]
        self._chk(library().fheram_bank_read_mix(self._h, C.byref(cm), *[_p(o) if o is not None else None for o in outs]))
        return tuple(outs)

    def _mix_reads(self, who, list, tables, regs, n_more):
        """the three read groups of read_mix / read_prepare_write_mix as the C struct, refused here as the library would refuse them;
        n_more: the entries the call has besides.  Returns (struct, the arrays it points to, (n_list, n_table, n_regs))."""
        members, addresses = (builtins_list(list[0]), builtins_list(list[1])) if list is not None else ([], [])
        tabs, tsels = (builtins_list(tables[0]), builtins_list(tables[1])) if tables is not None else ([], [])
        regfile, rsels = (regs[0], builtins_list(regs[1])) if regs is not None else (None, [])
        if len(addresses) != len(members) or len(tsels) != len(tabs):
            raise FheRamError(1, f"{who} takes as many addresses as members and as many selectors as tables, got {len(members)} / {len(addresses)} and {len(tabs)} / {len(tsels)}")
        nl, nt, nr = len(members), len(tabs), len(rsels)
        if nl + nt + nr + n_more > MIX_MAX:
            raise FheRamError(1, f"{who} takes at most MIX_MAX = {MIX_MAX} entries in all, got {nl + nt + nr + n_more}")
        if not all(isinstance(a, Address) for a in addresses):
            raise FheRamError(1, "every list entry must be an Address (a null address is refused)")
        if not all(isinstance(t, Table) for t in tabs) or not all(isinstance(s, Selector) for s in tsels + rsels):
            raise FheRamError(1, f"{who} takes Tables and Selectors")
        if nr and not isinstance(regfile, RegFile):
            raise FheRamError(1, f"the regs group of {who} takes a RegFile")
        members = [int(m) for m in members]
        for m in members:
            self._member(m)
        cm = _CMixReads()
        keep = []   # the arrays the struct points to

        def arr(ctype, values):
            a = (ctype * max(len(values), 1))(*values)
            keep.append(a)
            return a

        if nl:
            cm.members, cm.addrs, cm.n_list = arr(C.c_int, members), arr(C.c_void_p, [a._bank(self) for a in addresses]), nl
        if nt:
            cm.tables, cm.table_sels, cm.n_table = arr(C.c_void_p, [t._h for t in tabs]), arr(C.c_void_p, [s._h for s in tsels]), nt
        if nr:
            cm.regs, cm.reg_sels, cm.n_regs = regfile._h, arr(C.c_void_p, [s._h for s in rsels]), nr
        return cm, keep, (nl, nt, nr)

    def read_prepare_write_mix(self, list=None, tables=None, regs=None, prepare_list=None, prepare_regs=None, download: bool = True,
                               keys: Optional[EvaluationKeysPrepared] = None):
        """the reads of a step and the first halves of its writes under ONE top (fheram_bank_read_prepare_write_mix).
        list / tables / regs: the read groups of read_mix, all of which may be left out; prepare_list = (members, addresses): distinct
        members, as read_prepare_write_list; prepare_regs = (regfile, selector): as RegFile.read_prepare_write.  At least one of the two,
        and at most MIX_MAX entries in all (the register file counts 1).  Equals read_mix, read_prepare_write_list,
        RegFile.read_prepare_write in that order, in every output and in what is left on the bank; a member may be read and prepared in
        one call (the read sees the rows before the preparation), and so may the register file.  Returns (list, table, regs, prepared
        list, prepared regs): int64 [n][word_size][GLWE] per read group, the OLD words [n][word_size][GLWE] of the prepare list and the
        OLD register word [word_size][GLWE]; None for what is left out; download=False: no host wait, five times None."""
        pmembers, paddresses = (builtins_list(prepare_list[0]), builtins_list(prepare_list[1])) if prepare_list is not None else ([], [])
        pregfile, psel = prepare_regs if prepare_regs is not None else (None, None)
        npl, npr = len(pmembers), 1 if prepare_regs is not None else 0
        if len(paddresses) != npl:
            raise FheRamError(1, f"read_prepare_write_mix takes as many addresses as prepared members, got {npl} / {len(paddresses)}")
        if npl + npr < 1:
            raise FheRamError(1, "read_prepare_write_mix takes at least one preparation: no prepare list and no register file (that is read_mix)")
        cm, keep, counts = RamBank._mix_reads(self, "read_prepare_write_mix", list, tables, regs, npl + npr)
        if not all(isinstance(a, Address) for a in paddresses):
            raise FheRamError(1, "every prepare list entry must be an Address (a null address is refused)")
        if npr and not (isinstance(pregfile, RegFile) and isinstance(psel, Selector)):
            raise FheRamError(1, "prepare_regs of read_prepare_write_mix takes a RegFile and a Selector")
        pmembers = [int(m) for m in pmembers]
        for m in pmembers:
            self._member(m)
        if len(set(pmembers)) != npl:
            raise FheRamError(1, "the members of a prepare list are distinct: a RAM has one pending write")
        if keys is not None:
            self._use_keys(keys)
        cp = _CMixPrepares()
        if npl:
            am, aa = (C.c_int * npl)(*pmembers), (C.c_void_p * npl)(*[a._bank(self) for a in paddresses])
            keep += [am, aa]
            cp.members, cp.addrs, cp.n_list = am, aa, npl
        if npr:
            cp.regs, cp.reg_sel = pregfile._h, psel._h
        p = self.params
        shape = (p.word_size(), p.glwe_len())
        outs = [np.zeros((n,) + shape, dtype=np.int64) if (download and n) else None for n in counts + (npl,)]
        outs.append(np.zeros(shape, dtype=np.int64) if (download and npr) else None)
        self._chk(library().fheram_bank_read_prepare_write_mix(self._h, C.byref(cm), C.byref(cp), *[_p(o) if o is not None else None for o in outs]))
        return tuple(outs)

    def _host_words(self, host_words, slots):
        """host_words as int64, with the named slots inside it"""
        if host_words is None:
            return None
        hw = _i64(host_words)
        per = self.params.word_size() * self.params.glwe_len()
        if slots and (min(slots) < 0 or (max(slots) + 1) * per > hw.size):
            raise FheRamError(1, f"a host source names a slot outside host_words ({hw.size // per} slots of {self.params.word_size()} GLWEs)")
        return hw

    # -- the setup side: encrypt and decrypt on the bank's device, sampling on the host
    def _secret(self, sk):
        if not isinstance(sk, GLWESecret):
            raise FheRamError(1, "the bank's setup calls take a GLWESecret (GLWESecret(bank, sk))")
        return sk._h

    def _rows_draws(self, rows: int, source_xa, source_xe):
        """the draws of Ram::encrypt_sk for `rows` rows per word, in the reference's order (word-major, then row)"""
        p = self.params
        n, b2k = p.n(), p.basek()
        size = -(-p.k_glwe_ct() // b2k)
        ws = p.word_size()
        mask = source_xa.uniform_limbs(ws * rows * size * n)
        noise = source_xe.gaussian(ws * rows * n, noise_scale(p.k_glwe_ct(), b2k))
        return mask, noise

    def _one_row_encrypt(self, fn, obj, bits: int, data, sk, source_xa, source_xe):
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).ravel())
        skh = self._secret(sk)
        mask, noise = self._rows_draws(1, source_xa, source_xe)
        self._chk(fn(self._h, obj._h, skh, data.ctypes.data_as(C.POINTER(C.c_uint8)), data.size, _p(mask), _p(noise)))

    def _one_row_decrypt(self, fn, obj, bits: int, sk):
        skh = self._secret(sk)
        values = np.zeros(((1 << bits), self.params.word_size()), dtype=np.int32)
        worst = C.c_double()
        self._chk(fn(self._h, obj._h, skh, values.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(worst)))
        return values, float(worst.value)

    def encrypt_sk(self, member: int, data, sk: GLWESecret, source_xa, source_xe):
        """Ram::encrypt_sk (ram.rs:129-167) of one member, straight into its rows (fheram_bank_ram_encrypt_sk).  data: max_addr *
        word_size bytes; the sources draw in the reference's order, as Ram.encrypt_sk's."""
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).ravel())
        skh = self._secret(sk)
        mask, noise = self._rows_draws(self.params.rows(), source_xa, source_xe)
        self._chk(library().fheram_bank_ram_encrypt_sk(self._h, self._member(member), skh, data.ctypes.data_as(C.POINTER(C.c_uint8)), data.size,
                                                       _p(mask), _p(noise)))

    def glwe_encrypt_sk(self, sk: GLWESecret, n_glwe: int, size: int, k: int, pt, pt_col: int, source_xa, source_xe):
        """Ram.glwe_encrypt_sk on the bank's secret (fheram_bank_glwe_encrypt_sk)"""
        n = self.params.n()
        mask = source_xa.uniform_limbs(n_glwe * size * n)
        noise = source_xe.gaussian(n_glwe * n, noise_scale(k, self.params.basek()))
        out = np.zeros((n_glwe, size * 2 * n), dtype=np.int64)
        pt_size = 0
        if pt is not None:
            pt = _i64(pt).reshape(n_glwe, -1, n)
            pt_size = pt.shape[1]
        self._chk(library().fheram_bank_glwe_encrypt_sk(self._h, self._secret(sk), n_glwe, size, k, _p(pt) if pt is not None else None,
                                                        pt_size, pt_col, _p(mask), _p(noise), _p(out)))
        return out

    def glwe_decrypt(self, sk: GLWESecret, cts, size: int = 3):
        """Ram.glwe_decrypt on the bank's secret (fheram_bank_glwe_decrypt): normalised plaintext limbs [n_glwe][size][N]"""
        n = self.params.n()
        cts = _i64(cts).reshape(-1, size * 2 * n)
        pt = np.zeros((cts.shape[0], size, n), dtype=np.int64)
        self._chk(library().fheram_bank_glwe_decrypt(self._h, self._secret(sk), cts.shape[0], size, _p(cts), _p(pt)))
        return pt

    encrypt_word = Ram.encrypt_word      # (the example's encrypt_glwe: one GLWE per byte, through glwe_encrypt_sk above)
    decrypt_coeff = Ram.decrypt_coeff    # (the example's decrypt_glwe + noise metric on downloaded ciphertexts, through glwe_decrypt above)

    def decrypt_sources(self, sk: GLWESecret, srcs, wants=None):
        """decrypts and decodes, on the device, coefficient 0 of the words `srcs` name (Src.member / list / select / regs / regs_old /
        table; fheram_bank_source_decrypt): (values, log2 noise), int64 and float64 [n][word_size].  wants: [n][word_size] expected values,
        or None (the decoded value itself is the expectation).  Nothing on the device changes."""
        srcs = list(srcs)
        if not srcs or not all(isinstance(s, Src) for s in srcs):
            raise FheRamError(1, "decrypt_sources takes a non-empty list of Src")
        n, ws = len(srcs), self.params.word_size()
        if wants is not None:
            wants = _i64(wants)
            if wants.size != n * ws:
                raise FheRamError(1, f"wants must hold {n} x {ws} values")
        values = np.zeros((n, ws), dtype=np.int64)
        noise = np.zeros((n, ws), dtype=np.float64)
        arr = (_CSelectSrc * n)(*[_CSelectSrc(s.kind, s.index) for s in srcs])
        self._chk(library().fheram_bank_source_decrypt(self._h, self._secret(sk), arr, n, _p(wants) if wants is not None else None, _p(values),
                                                       noise.ctypes.data_as(C.POINTER(C.c_double))))
        return values, noise

    def decrypt(self, member: int, sk: GLWESecret):
        """every word of one member, decrypted and decoded on the device (fheram_bank_ram_decrypt): (values int32 [max_addr][word_size],
        worst log2 noise against each coefficient's own decoded value)"""
        skh = self._secret(sk)
        values = np.zeros((self.params.max_addr(), self.params.word_size()), dtype=np.int32)
        worst = C.c_double()
        self._chk(library().fheram_bank_ram_decrypt(self._h, self._member(member), skh, values.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(worst)))
        return values, float(worst.value)

    def selftest_fail_select_alloc(self, nth: int):
        """self-test: the nth device allocation the select's buffers ask for from now on fails once (0: none)"""
        self._chk(library().fheram_bank_selftest_fail_select_alloc(self._h, int(nth)))

    def result(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """the results of each member's last read / read_prepare_write"""
        first, n = self._range(first, self.n_members - int(first) if n is None else n)
        p = self.params
        out = np.zeros((n, p.word_size(), p.glwe_len()), dtype=np.int64)
        self._chk(library().fheram_bank_result_download(self._h, first, n, _p(out)))
        return out

    def sync(self):
        self._chk(library().fheram_bank_sync(self._h))

    def roundoff_max(self, check: bool = True) -> float:
        """the largest |x - rint(x)| any inverse transform of the bank has rounded away; raises PRECISION above 3/8 unless check=False"""
        m = C.c_double()
        rc = library().fheram_bank_roundoff_max(self._h, C.byref(m))
        if rc != 0 and (check or rc != 8):
            self._chk(rc)
        return float(m.value)

    def roundoff_reset(self):
        self._chk(library().fheram_bank_roundoff_reset(self._h))

    def tail_stats(self):
        n, f = C.c_uint64(), C.c_uint64()
        self._chk(library().fheram_bank_tail_stats(self._h, C.byref(n), C.byref(f)))
        return {"launches": int(n.value), "fallbacks": int(f.value)}

    def mid_stats(self):
        n, f = C.c_uint64(), C.c_uint64()
        self._chk(library().fheram_bank_mid_stats(self._h, C.byref(n), C.byref(f)))
        return {"launches": int(n.value), "fallbacks": int(f.value)}

    def profile_enable(self, on=True):
        self._chk(library().fheram_bank_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._chk(library().fheram_bank_profile_reset(self._h))

    def profile_get(self, cls: str):
        n, b, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        self._chk(library().fheram_bank_profile_get(self._h, cls.encode(), C.byref(n), C.byref(b), C.byref(ms)))
        return {"launches": int(n.value), "blocks": int(b.value), "ms": float(ms.value)}
