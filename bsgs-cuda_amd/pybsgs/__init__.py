"""pybsgs -- thin ctypes binding of libbsgs_hip.so (include/bsgs_hip.h).

Plumbing only: every call goes straight to the C-ABI; there is NO CPU fallback.  Importing works
without a GPU (so CPU-only checks can verify the exported symbols); opening a device without an
MI355X raises BsgsError.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("BSGS_LIB_PATH") or os.path.join(PKG_ROOT, "build", "libbsgs_hip.so")   # override: A/B of alternative builds

TABLE_AUTO, TABLE_CSR, TABLE_LINES64, TABLE_LINES128, TABLE_LINES64_LIST, TABLE_LINES128_LIST = 0, 1, 2, 3, 4, 5
ERR_OVERFLOW = -5
ERR_DEGENERATE = -6
FLAG_REFERENCE_QUIRKS = 1

# every symbol include/bsgs_hip.h declares (checked by tests/test_abi.py)
NATIVE_SYMBOLS = [
    "bsgs_last_error", "bsgs_version", "bsgs_build_info", "bsgs_dev_count", "bsgs_dev_open", "bsgs_dev_close", "bsgs_dev_name",
    "bsgs_dev_meminfo", "bsgs_dev_cu_count", "bsgs_upload_g2", "bsgs_upload_g2_device", "bsgs_generate_g2",
    "bsgs_download_g2", "bsgs_upload_htgpu", "bsgs_upload_htgpu_device", "bsgs_table_info", "bsgs_step", "bsgs_run",
    "bsgs_enqueue", "bsgs_collect", "bsgs_dev_stream", "bsgs_steps_per_tile", "bsgs_selftest_fe", "bsgs_selftest_xs",
    "bsgs_bench_random_read", "bsgs_bench_stream", "bsgs_bench_modmul", "bsgs_set_tiles_per_launch", "bsgs_launch_count", "bsgs_build_baby_tables", "bsgs_build_baby_tables_device", "bsgs_build_baby_table_ext", "bsgs_ext_overflow_capacity", "bsgs_build_baby_table_ext_device", "bsgs_install_table_ext_device", "bsgs_profile_phases",
    "bsgs_set_walk", "bsgs_enqueue_walk", "bsgs_run_walk", "bsgs_walk_centres", "bsgs_set_flags", "bsgs_quirk_count", "bsgs_broadcast_tables",
    "bsgs_tiles_per_launch", "bsgs_engine_geometry", "bsgs_run_digest", "bsgs_selftest_lo64", "bsgs_compat_stats", "bsgs_debug_buffers", "bsgs_alloc_stats", "bsgs_tune_placement", "bsgs_chain_placement", "bsgs_chain_grades", "bsgs_debug_grade_rule", "bsgs_debug_xcd_profile",
    "bsgs_table_checksum", "bsgs_sample_g2", "bsgs_alloc_table_ext_recv", "bsgs_debug_last_kernel", "bsgs_compat_stats_ex", "bsgs_debug_table_owner", "bsgs_prepare", "bsgs_debug_last_batching", "bsgs_debug_last_tiles_per_block", "bsgs_debug_narrow_batching",
    "bsgs_table_census", "bsgs_table_lookup", "bsgs_broadcast_tables_ex", "bsgs_startup_ext_tables", "bsgs_build_baby_table_ext_slice", "bsgs_build_overflow_set", "bsgs_debug_fabric_selftest", "bsgs_share_tables",
    "bsgs_kangaroo_setup", "bsgs_kangaroo_upload", "bsgs_kangaroo_upload_list", "bsgs_kangaroo_download", "bsgs_kangaroo_run", "bsgs_kangaroo_geometry", "bsgs_kangaroo_seed", "bsgs_kangaroo_setup_sym", "bsgs_kangaroo_setup_sym_keys",
    "bsgs_kangaroo_set_keys", "bsgs_kangaroo_seed_keys", "bsgs_kangaroo_verify", "bsgs_kangaroo_verify_points", "bsgs_selftest_fe3",
    "bsgs_kangaroo_tames_image", "bsgs_kangaroo_tames_install", "bsgs_kangaroo_run_tames", "bsgs_kangaroo_tames_install_keys", "bsgs_kangaroo_run_tames_keys",
    "bsgs_kangaroo_tames_gen_begin", "bsgs_kangaroo_run_tames_gen", "bsgs_kangaroo_tames_gen_insert", "bsgs_kangaroo_tames_gen_read", "bsgs_kangaroo_tames_gen_end",
    "bsgs_kangaroo_tames_gen_load", "bsgs_kangaroo_tames_gen_read_sorted",
    "bsgs_kangaroo_dptable_begin", "bsgs_kangaroo_run_dptable", "bsgs_kangaroo_dptable_insert", "bsgs_kangaroo_dptable_load", "bsgs_kangaroo_dptable_read", "bsgs_kangaroo_dptable_end",
    "bsgs_kangaroo_dptable_begin_keys", "bsgs_kangaroo_run_dptable_keys", "bsgs_kangaroo_dptable_insert_keys",
    "bsgs_kangaroo_dptable_begin_shard", "bsgs_kangaroo_run_dptable_shard", "bsgs_kangaroo_dptable_insert_shard",
]
# exported by the TEST build only (build/libbsgs_hip_test.so = the shipped objects + csrc/test_hooks.hip; include/bsgs_hip.h under BSGS_TEST_HOOKS)
TEST_HOOK_SYMBOLS = ["bsgs_debug_corrupt_table", "bsgs_debug_realloc", "bsgs_debug_launch_split", "bsgs_debug_last_split"]
TEST_LIB_PATH = os.path.join(PKG_ROOT, "build", "libbsgs_hip_test.so")
COMPAT_SYMBOLS = [
    "cuInit", "cuDeviceGetCount", "cuDeviceGet", "cuDeviceGetName", "cuDeviceTotalMem_v2", "cuDeviceComputeCapability",
    "cuDeviceGetAttribute", "cuCtxCreate_v2", "cuCtxDestroy_v2", "cuCtxSynchronize", "cuMemGetInfo_v2", "cuModuleLoadData",
    "cuModuleGetFunction", "cuModuleGetGlobal_v2", "cuFuncSetCacheConfig", "cuFuncSetBlockShape", "cuParamSetSize",
    "cuParamSeti", "cuMemAlloc_v2", "cuMemFree_v2", "cuMemcpyHtoD_v2", "cuMemcpyDtoH_v2", "cuLaunchGrid",
    # declared by the reference's Import block but never called by v1.9.7 (exported so that the unchanged block links)
    "cuDeviceTotalMem", "cuCtxCreate", "cuCtxDestroy", "cuMemAlloc", "cuMemFree", "cuMemcpyHtoD", "cuMemcpyDtoH", "cuModuleGetGlobal",
    "cuModuleLoad", "cuParamSetv", "cuLaunchGridAsync", "cuLaunch", "cuFuncSetSharedSize", "cuFuncGetAttribute", "cuGetErrorName",
    "cuEventCreate", "cuEventDestroy", "cuEventQuery", "cuEventRecord", "cuEventSynchronize", "cuStreamCreate", "cuStreamCreate_v2",
    "cuStreamDestroy", "cuStreamSynchronize", "cuStreamQuery",
]


class BsgsError(RuntimeError):
    pass


class Hit(C.Structure):
    _fields_ = [("code", C.c_uint32), ("idx", C.c_uint32)]


class HitEx(C.Structure):
    _fields_ = [("code", C.c_uint32), ("idx", C.c_uint32), ("tile", C.c_uint32), ("reserved", C.c_uint32)]


class KangarooState(C.Structure):
    _fields_ = [("x", C.c_uint8 * 32), ("y", C.c_uint8 * 32), ("d", C.c_uint8 * 16), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class KangarooRecord(C.Structure):
    _fields_ = [("x", C.c_uint8 * 32), ("d", C.c_uint8 * 16), ("kangaroo", C.c_uint32), ("flags", C.c_uint32), ("step", C.c_uint32), ("reserved", C.c_uint32)]


# bsgs_selftest_fe3: ops of the three-operand field selftest, and fe_inv_block alone (four waves per block: the strides of the kangaroo, seed and tile kernels;
# two waves: the tile kernels' two strides)
FE3_SQR_ADD2, FE3_NEG, FE3_CANON, FE3_ADD, FE3_SUB, FE3_MUL, FE3_SQR, FE3_INV = range(8)
FE3_IS_P, FE3_IS_ZERO, FE3_EQ, FE3_ADD_IS_P, FE3_SUB_IS_ZERO = range(8, 13)
FE3_INV_BLOCK_KANG, FE3_INV_BLOCK_SEED, FE3_INV_BLOCK_TILE, FE3_INV_BLOCK2_TILE, FE3_INV_BLOCK2_TILE_PAIR128 = range(16, 21)

KANGAROO_JUMPS, KANGAROO_WILD, KANGAROO_DEAD = 64, 1, 0x80000000
KANGAROO_NEG, KANGAROO_CYCLE = 2, 4                # the symmetric walk (kangaroo_setup_sym)
KANGAROO_GEN_DEAD, KANGAROO_GEN_DUPLICATE, KANGAROO_GEN_TAG_ZERO, KANGAROO_GEN_FULL = range(4)   # why the growing tame table hands a record back
KANGAROO_DPT_DEAD, KANGAROO_DPT_DUPLICATE, KANGAROO_DPT_TAG_ZERO, KANGAROO_DPT_FULL, KANGAROO_DPT_STORED = range(5)   # the distinguished-point table's hand-backs
KANGAROO_DPT_KEY_SHIFT = 8   # the table for a key list: a hand-back's `reserved` = reason | key << 8; an entry's owner: 0 tame, 1 + key wild, bit 31 NEG
KANGAROO_DPT_MAX_SHARDS = 16   # the table divided over engines: shard(tag) = ((tag >> 48) * shards) >> 16
KANGAROO_KEY_SHIFT, KANGAROO_MAX_KEYS = 8, 65535   # many keys in one herd (kangaroo_set_keys): a wild kangaroo's key index, 16 bits of its flags

_lib = None


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (same SONAME as /opt/rocm's) and asks for it by a name the
    system copy does not answer to: if libbsgs_hip.so pulled in /opt/rocm's first, a later `import torch` loads a SECOND runtime and finds
    "No HIP GPUs".  So when torch is installed but not imported yet, its copy is loaded first (by path, globally) and libbsgs_hip.so binds
    to it through the SONAME -- the arrangement every `import torch; import pybsgs` process has anyway.  BSGS_NO_TORCH_HIP_PRELOAD=1 skips it."""
    import sys
    if "torch" in sys.modules or os.environ.get("BSGS_NO_TORCH_HIP_PRELOAD") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load the HIP extension; fail loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BsgsError("HIP extension missing: %s (run `make -C bsgs-cuda_amd` or __graft_entry__.build())" % LIB_PATH)
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        vp, u8p = C.c_void_p, C.c_char_p
        L.bsgs_last_error.restype = C.c_char_p
        L.bsgs_version.restype = C.c_char_p
        L.bsgs_build_info.restype = C.c_char_p
        sig = {
            "bsgs_dev_count": [C.POINTER(C.c_int)],
            "bsgs_dev_open": [C.c_int, C.POINTER(vp)],
            "bsgs_dev_close": [vp],
            "bsgs_dev_name": [vp, C.c_char_p, C.c_int],
            "bsgs_dev_meminfo": [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
            "bsgs_dev_cu_count": [vp, C.POINTER(C.c_int)],
            "bsgs_upload_g2": [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32],
            "bsgs_upload_g2_device": [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32],
            "bsgs_generate_g2": [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32],
            "bsgs_download_g2": [vp, vp, C.c_size_t],
            "bsgs_upload_htgpu": [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32],
            "bsgs_upload_htgpu_device": [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32],
            "bsgs_table_info": [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
            "bsgs_step": [vp, u8p, u8p, C.POINTER(Hit), C.c_uint32, C.POINTER(C.c_uint32)],
            "bsgs_run": [vp, u8p, C.c_uint32, C.POINTER(HitEx), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float)],
            "bsgs_enqueue": [vp, u8p, C.c_uint32],
            "bsgs_collect": [vp, C.POINTER(HitEx), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float)],
            "bsgs_dev_stream": [vp, C.POINTER(vp)],
            "bsgs_steps_per_tile": [vp, C.POINTER(C.c_uint64)],
            "bsgs_selftest_fe": [vp, C.c_int, u8p, u8p, vp, C.c_uint32],
            "bsgs_selftest_fe3": [vp, C.c_int, C.c_int, u8p, u8p, u8p, vp, C.c_uint32],
            "bsgs_selftest_xs": [vp, u8p, u8p, C.c_uint64, C.c_uint32, vp],
            "bsgs_bench_random_read": [vp, C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)],
            "bsgs_bench_modmul": [vp, C.POINTER(C.c_double)],
            "bsgs_bench_stream": [vp, C.c_int, C.c_uint64, C.POINTER(C.c_double)],
            "bsgs_set_tiles_per_launch": [vp, C.c_uint32],
            "bsgs_launch_count": [vp, C.POINTER(C.c_uint64)],
            "bsgs_build_baby_tables": [vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32],
            "bsgs_build_baby_tables_device": [vp, C.c_uint64, C.c_uint32, vp, vp],
            "bsgs_build_baby_table_ext": [vp, C.c_uint64, C.c_uint32, C.c_uint32],
            "bsgs_ext_overflow_capacity": [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)],
            "bsgs_build_baby_table_ext_device": [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
            "bsgs_install_table_ext_device": [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32],
            "bsgs_alloc_table_ext_recv": [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)],
            "bsgs_debug_last_kernel": [vp, C.c_char_p, C.c_int],
            "bsgs_table_checksum": [vp, C.POINTER(C.c_uint64)],
            "bsgs_table_census": [vp, C.POINTER(C.c_uint64)],
            "bsgs_broadcast_tables_ex": [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)],
            "bsgs_startup_ext_tables": [C.POINTER(vp), C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp],
            "bsgs_build_baby_table_ext_slice": [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
            "bsgs_build_overflow_set": [vp, vp, C.c_uint64, vp, C.c_uint64],
            "bsgs_debug_fabric_selftest": [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)],
            "bsgs_table_lookup": [vp, vp, C.c_uint64, vp],
            "bsgs_sample_g2": [vp, vp, C.c_uint32, vp],
            "bsgs_debug_corrupt_table": [vp, C.c_uint64, C.c_uint32],
            "bsgs_debug_table_owner": [vp, C.POINTER(C.c_int)],
            "bsgs_prepare": [vp],
            "bsgs_profile_phases": [vp, u8p, C.c_uint32, C.POINTER(C.c_float)],
            "bsgs_set_walk": [vp, u8p, u8p],
            "bsgs_enqueue_walk": [vp, C.c_uint64, C.c_uint32],
            "bsgs_run_walk": [vp, C.c_uint64, C.c_uint32, C.POINTER(HitEx), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float)],
            "bsgs_walk_centres": [vp, C.c_uint64, C.c_uint32, vp],
            "bsgs_set_flags": [vp, C.c_uint32],
            "bsgs_quirk_count": [vp, C.POINTER(C.c_uint32)],
            "bsgs_broadcast_tables": [C.POINTER(vp), C.c_int],
            "bsgs_share_tables": [vp, vp],
            "bsgs_tiles_per_launch": [vp, C.POINTER(C.c_uint32)],
            "bsgs_engine_geometry": [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
            "bsgs_debug_last_batching": [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
            "bsgs_debug_last_tiles_per_block": [vp, C.POINTER(C.c_uint32)],
            "bsgs_debug_narrow_batching": [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)],
            "bsgs_run_digest": [vp, u8p, C.c_uint32, vp, C.POINTER(HitEx), C.c_uint32, C.POINTER(C.c_uint32)],
            "bsgs_selftest_lo64": [vp, u8p, u8p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)],
            "bsgs_debug_buffers": [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)],
            "bsgs_debug_realloc": [vp, C.c_int, C.c_uint64],
            "bsgs_debug_xcd_profile": [vp, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_float)],
            "bsgs_kangaroo_setup": [vp, u8p, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32],
            "bsgs_kangaroo_setup_sym": [vp, u8p, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32],
            "bsgs_kangaroo_setup_sym_keys": [vp, u8p, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32],
            "bsgs_kangaroo_upload": [vp, C.c_uint32, C.c_uint32, C.POINTER(KangarooState)],
            "bsgs_kangaroo_upload_list": [vp, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(KangarooState)],
            "bsgs_kangaroo_download": [vp, C.c_uint32, C.c_uint32, C.POINTER(KangarooState)],
            "bsgs_kangaroo_run": [vp, C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)],
            "bsgs_kangaroo_geometry": [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
            "bsgs_kangaroo_set_keys": [vp, u8p, C.c_uint32],
            "bsgs_kangaroo_seed_keys": [vp, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, u8p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
            "bsgs_kangaroo_verify": [vp, u8p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32],
            "bsgs_kangaroo_verify_points": [vp, u8p, C.c_uint32, u8p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32],
            "bsgs_kangaroo_seed": [vp, u8p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, u8p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
            "bsgs_kangaroo_tames_image": [C.POINTER(C.c_uint64), C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)],
            "bsgs_kangaroo_tames_install": [vp, C.POINTER(C.c_uint64), C.c_uint64],
            "bsgs_kangaroo_run_tames": [vp, C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)],
            "bsgs_kangaroo_tames_install_keys": [vp, C.POINTER(C.c_uint64), C.c_uint64],
            "bsgs_kangaroo_tames_gen_begin": [vp, C.c_uint64],
            "bsgs_kangaroo_run_tames_gen": [vp, C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_float)],
            "bsgs_kangaroo_tames_gen_insert": [vp, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)],
            "bsgs_kangaroo_tames_gen_read": [vp, C.POINTER(C.c_uint64), vp, C.c_uint64, C.POINTER(C.c_uint64)],
            "bsgs_kangaroo_tames_gen_end": [vp],
            "bsgs_kangaroo_tames_gen_load": [vp, vp, vp, C.c_uint64] + [C.POINTER(C.c_uint64)] * 5,
            "bsgs_kangaroo_tames_gen_read_sorted": [vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)],
            "bsgs_kangaroo_dptable_begin": [vp, C.c_uint64],
            "bsgs_kangaroo_run_dptable": [vp, C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_float)],
            "bsgs_kangaroo_dptable_insert": [vp, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint64)],
            "bsgs_kangaroo_dptable_load": [vp, vp, C.c_uint64] + [C.POINTER(C.c_uint64)] * 5,
            "bsgs_kangaroo_dptable_read": [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)],
            "bsgs_kangaroo_dptable_end": [vp],
            "bsgs_kangaroo_dptable_begin_keys": [vp, C.c_uint64],
            "bsgs_kangaroo_run_dptable_keys": [vp, C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_float)],
            "bsgs_kangaroo_dptable_insert_keys": [vp, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32),
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
            "bsgs_kangaroo_dptable_begin_shard": [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32],
            "bsgs_kangaroo_run_dptable_shard": [vp, C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(KangarooRecord), C.c_uint32,
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)],
            "bsgs_kangaroo_dptable_insert_shard": [vp, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32),
                                                   C.POINTER(KangarooRecord), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
            "bsgs_kangaroo_run_tames_keys": [vp, C.c_uint32, C.POINTER(KangarooRecord), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_float)],
        }
        for name, args in sig.items():
            fn = getattr(L, name, None)
            if fn is None:                       # an older build loaded through BSGS_LIB_PATH for an A/B run: the call site raises if it is ever needed
                continue
            fn.argtypes = args
            fn.restype = C.c_int
        _lib = L
    return _lib


def _chk(rc, allow_overflow=False):
    if rc == 0 or (allow_overflow and rc == ERR_OVERFLOW):
        return rc
    raise BsgsError("bsgs error %d: %s" % (rc, lib().bsgs_last_error().decode()))


def le32(v):
    return int(v).to_bytes(32, "little")


def kangaroo_tames_image(tags):
    """the device image of a tame table (include/bsgs_hip.h, "Kangaroo, tame table") from its tags, the low 64 bits of x in entry order: (bytes, lines).
    Needs no device; a tag that occurs twice raises"""
    n = len(tags)
    arr = (C.c_uint64 * max(1, n))(*tags)
    lines = C.c_uint64()
    _chk(lib().bsgs_kangaroo_tames_image(arr, n, None, 0, C.byref(lines)))
    buf = C.create_string_buffer(lines.value * 64)
    _chk(lib().bsgs_kangaroo_tames_image(arr, n, buf, len(buf), C.byref(lines)))
    return buf.raw, lines.value


def build_info():
    """the -D switches the loaded library was built with ("" = the shipped build; "WRONG-RESULTS:..." = a timing experiment)"""
    return lib().bsgs_build_info().decode()


def broadcast_tables(devices):
    """replicas of devices[0]'s giants and table on the other Device objects (device-to-device copies; the same GPU may appear twice)"""
    arr = (C.c_void_p * len(devices))(*[d.h for d in devices])
    _chk(lib().bsgs_broadcast_tables(arr, len(devices)))


def share_tables(owner, twin):
    """two engines on one GPU: `twin` probes `owner`'s table in place (borrowed) and gets its own copy of the giants"""
    _chk(lib().bsgs_share_tables(owner.h, twin.h))


TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_PEER = 0, 1, 2
STARTUP_BROADCAST, STARTUP_LOCAL, STARTUP_ALLGATHER = 0, 1, 2


class StartupReport(C.Structure):
    _fields_ = [("alloc_s", C.c_double), ("build_s", C.c_double), ("transfer_s", C.c_double), ("set_s", C.c_double), ("install_s", C.c_double),
                ("prepare_s", C.c_double), ("total_s", C.c_double), ("bytes_received", C.c_uint64), ("strategy", C.c_uint32), ("transport", C.c_uint32)]


def startup_ext_tables(devices, w, htsz, layout, strategy, transport=TRANSPORT_AUTO):
    """extended table on every Device of one process by one of the three start-up strategies (include/bsgs_hip.h BSGS_STARTUP_*); returns one dict per engine"""
    arr = (C.c_void_p * len(devices))(*[d.h for d in devices])
    rep = (StartupReport * len(devices))()
    _chk(lib().bsgs_startup_ext_tables(arr, len(devices), w, htsz, layout, strategy, transport, C.cast(rep, C.c_void_p)))
    return [{k: getattr(r, k) for k, _ in StartupReport._fields_} for r in rep]


def broadcast_tables_ex(devices, transport=TRANSPORT_AUTO, what=3):
    """replicas of devices[0]'s giants (what & 1) and table (what & 2) on the other Devices; returns (transport used, seconds)"""
    arr = (C.c_void_p * len(devices))(*[d.h for d in devices])
    used, secs = C.c_uint32(), C.c_double()
    _chk(lib().bsgs_broadcast_tables_ex(arr, len(devices), transport, what, C.byref(used), C.byref(secs)))
    return used.value, secs.value


def fabric_selftest(devices, transport, nbytes):
    """(mismatching words after the broadcast, after the all-gather, transport used) of the transport test (bsgs_debug_fabric_selftest)"""
    arr = (C.c_void_p * len(devices))(*[d.h for d in devices])
    bad, used = (C.c_uint64 * 2)(), C.c_uint32()
    _chk(lib().bsgs_debug_fabric_selftest(arr, len(devices), transport, nbytes, bad, C.byref(used)))
    return int(bad[0]), int(bad[1]), used.value


def alloc_stats():
    """(bytes of big buffers obtained physically contiguous, bytes obtained as ordinary pages) by this process so far"""
    a, b = C.c_uint64(), C.c_uint64()
    lib().bsgs_alloc_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    _chk(lib().bsgs_alloc_stats(C.byref(a), C.byref(b)))
    return a.value, b.value


def device_count():
    n = C.c_int(0)
    _chk(lib().bsgs_dev_count(C.byref(n)))
    return n.value


class Device:
    """One GPU, mirroring the reference's per-GPU driver thread `cuda()` (1_9_7File.pb:2095-2553)."""

    def __init__(self, device_id=0):
        self.h = C.c_void_p()
        _chk(lib().bsgs_dev_open(device_id, C.byref(self.h)))
        self.L = lib()
        self._kang_keyed = False               # the herd is one of kangaroo_setup_sym_keys: states carry a key
        self._kang_cap = 0                     # record capacity of the herd (kangaroo_setup*)
        self._dpt_shards = 1                   # shards of the table begun by kangaroo_dptable_begin_shard

    def close(self):
        if self.h:
            self.L.bsgs_dev_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def name(self):
        buf = C.create_string_buffer(256)
        _chk(self.L.bsgs_dev_name(self.h, buf, 256))
        return buf.value.decode()

    def meminfo(self):
        f, t = C.c_uint64(), C.c_uint64()
        _chk(self.L.bsgs_dev_meminfo(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def upload_g2(self, image, t, b, p):
        buf = C.create_string_buffer(image, len(image)) if isinstance(image, (bytes, bytearray)) else image
        _chk(self.L.bsgs_upload_g2(self.h, C.cast(buf, C.c_void_p), t, b, p))

    def upload_g2_device(self, dptr, t, b, p):
        _chk(self.L.bsgs_upload_g2_device(self.h, C.c_void_p(dptr), t, b, p))

    def generate_g2(self, ax, ay, t, b, p):
        _chk(self.L.bsgs_generate_g2(self.h, le32(ax) + le32(ay), t, b, p))

    def download_g2(self, nbytes):
        buf = C.create_string_buffer(nbytes)
        _chk(self.L.bsgs_download_g2(self.h, C.cast(buf, C.c_void_p), nbytes))
        return buf.raw

    def upload_htgpu(self, image, ht_items, w, layout=TABLE_AUTO):
        buf = C.create_string_buffer(image, len(image)) if isinstance(image, (bytes, bytearray)) else image
        _chk(self.L.bsgs_upload_htgpu(self.h, C.cast(buf, C.c_void_p), ht_items, w, layout))

    def upload_htgpu_device(self, dptr, ht_items, w, layout=TABLE_AUTO):
        _chk(self.L.bsgs_upload_htgpu_device(self.h, C.c_void_p(dptr), ht_items, w, layout))

    def build_baby_tables(self, w, htsz, want_gpu=True, want_cpu=True, install_layout=0xFFFFFFFF):
        items = 1 << htsz
        g = C.create_string_buffer(4 * (items + 1) + 4 * w) if want_gpu else None
        c = C.create_string_buffer(4 * (items + 1) + 8 * w) if want_cpu else None
        _chk(self.L.bsgs_build_baby_tables(self.h, w, htsz, C.cast(g, C.c_void_p) if g else None,
                                           C.cast(c, C.c_void_p) if c else None, install_layout))
        return (g.raw if g else None), (c.raw if c else None)

    def build_baby_tables_device(self, w, htsz, htgpu_dptr, htcpu_dptr=None):
        _chk(self.L.bsgs_build_baby_tables_device(self.h, w, htsz, C.c_void_p(htgpu_dptr) if htgpu_dptr else None,
                                                  C.c_void_p(htcpu_dptr) if htcpu_dptr else None))

    def build_baby_table_ext(self, w, htsz, layout=TABLE_LINES64_LIST):
        """k*G, k = 1..w (w up to 2^36) straight into bucket lines + overflow list on the device (no CSR, no positions)"""
        _chk(self.L.bsgs_build_baby_table_ext(self.h, w, htsz, layout))

    def ext_overflow_capacity(self, w, htsz, layout=TABLE_LINES64_LIST):
        cap = C.c_uint64(0)
        _chk(self.L.bsgs_ext_overflow_capacity(w, htsz, layout, C.byref(cap)))
        return cap.value

    def build_baby_table_ext_device(self, w, htsz, layout, lines_dptr, ovf_dptr, ovf_cap):
        """build into caller-owned device buffers (source of an RCCL broadcast); returns (ovf_n, overflow_buckets)"""
        n, ob = C.c_uint64(0), C.c_uint64(0)
        _chk(self.L.bsgs_build_baby_table_ext_device(self.h, w, htsz, layout, C.c_void_p(lines_dptr), C.c_void_p(ovf_dptr), ovf_cap, C.byref(n), C.byref(ob)))
        return n.value, ob.value

    def build_baby_table_ext_slice(self, w, htsz, layout, lines_dptr, part, nparts, list_dptr, list_cap):
        """the lines of 1/nparts of the buckets, in place inside the full line buffer; returns (entries in the slice's overflow list, over-full lines of the slice)"""
        n, ob = C.c_uint64(0), C.c_uint64(0)
        _chk(self.L.bsgs_build_baby_table_ext_slice(self.h, w, htsz, layout, C.c_void_p(lines_dptr), part, nparts, C.c_void_p(list_dptr), list_cap, C.byref(n), C.byref(ob)))
        return n.value, ob.value

    def build_overflow_set(self, list_dptr, n, set_dptr, slots):
        _chk(self.L.bsgs_build_overflow_set(self.h, C.c_void_p(list_dptr), n, C.c_void_p(set_dptr), slots))

    def install_table_ext_device(self, lines_dptr, ovf_dptr, ovf_n, overflow_buckets, w, htsz, layout):
        _chk(self.L.bsgs_install_table_ext_device(self.h, C.c_void_p(lines_dptr), C.c_void_p(ovf_dptr), ovf_n, overflow_buckets, w, htsz, layout))

    def alloc_table_ext_recv(self, w, htsz, layout):
        """engine-owned receive buffers for a broadcast extended table: (lines_dptr, ovf_dptr, ovf_cap slots)"""
        lines, ovf, cap = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _chk(self.L.bsgs_alloc_table_ext_recv(self.h, w, htsz, layout, C.byref(lines), C.byref(ovf), C.byref(cap)))
        return lines.value, ovf.value, cap.value

    def prepare(self):
        _chk(self.L.bsgs_prepare(self.h))

    def table_checksum(self):
        """device-side 64-bit checksums of (bucket lines, overflow set, CSR image, giants): equal across byte-identical replicas"""
        s = (C.c_uint64 * 4)()
        _chk(self.L.bsgs_table_checksum(self.h, s))
        return [int(x) for x in s]

    def table_census(self):
        """one streaming pass over the installed table (the reference's checkHT / checkHTpack, 1_9_7File.pb:3599-3627, 3101-3134): what it holds, and whether
        entries in lines + keys in the overflow set - duplicates equals w"""
        c = (C.c_uint64 * 8)()
        _chk(self.L.bsgs_table_census(self.h, c))
        names = ("line_entries", "overfull_lines", "set_keys", "duplicates", "malformed_lines", "unsorted_lines", "w", "total")
        return dict(zip(names, (int(x) for x in c)))

    def table_lookup(self, keys64):
        """batched membership through the shipped probe: keys64 = iterable of 64-bit keys (low 64 bits of x) -> list of bool"""
        import array
        a = array.array("Q", keys64)
        n = len(a)
        if not n:
            return []
        out = (C.c_uint8 * n)()
        addr, _ = a.buffer_info()
        _chk(self.L.bsgs_table_lookup(self.h, C.c_void_p(addr), n, C.cast(out, C.c_void_p)))
        return [bool(x) for x in out]

    def _test_hook(self, name):
        fn = getattr(self.L, name, None)
        if fn is None:
            raise BsgsError("%s is a TEST hook: it lives in %s only (set BSGS_LIB_PATH to it before pybsgs loads its library); the shipped library does not export it" % (name, TEST_LIB_PATH))
        return fn

    def debug_corrupt_table(self, byte_offset, xor_mask=1):
        """TEST BUILD hook: flip bits of one byte of the installed table (what the verification must catch)"""
        _chk(self._test_hook("bsgs_debug_corrupt_table")(self.h, byte_offset, xor_mask))

    def debug_last_split(self):
        """TEST BUILD hook: first tile of part 1 of the most recent launch (two kernels on two streams, bsgs_hip.hip launch_tiles), 0 = it was one kernel"""
        n0 = C.c_uint32()
        fn = self._test_hook("bsgs_debug_last_split")
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        _chk(fn(self.h, C.byref(n0)))
        return n0.value

    def sample_g2(self, indices):
        """giants by number as (x, y) integer pairs (what a host compares with (i + 1) * ADDPUBG before it searches: checkGiantArr 1_9_7File.pb:1524-1559)"""
        import array
        a = array.array("Q", indices)
        n = len(a)
        if not n:
            return []
        out = C.create_string_buffer(64 * n)
        addr, _ = a.buffer_info()
        _chk(self.L.bsgs_sample_g2(self.h, C.c_void_p(addr), n, C.cast(out, C.c_void_p)))
        raw = out.raw
        return [(int.from_bytes(raw[64 * i:64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "little")) for i in range(n)]

    def table_owned(self):
        v = C.c_int()
        _chk(self.L.bsgs_debug_table_owner(self.h, C.byref(v)))
        return bool(v.value)

    def last_kernel(self):
        buf = C.create_string_buffer(128)
        _chk(self.L.bsgs_debug_last_kernel(self.h, buf, 128))
        return buf.value.decode()

    def last_batching(self):
        """(threads, giants per thread) of the most recent tile launch: engine_geometry() for launches that fill the GPU, more threads x shorter
        batches for small ones (bsgs_hip.hip pick_batching)"""
        a, b = C.c_uint32(), C.c_uint32()
        _chk(self.L.bsgs_debug_last_batching(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_tiles_per_block(self):
        """tiles per block of the most recent tile launch: 2 when the quad-chain kernel walked two tiles per block (bsgs_hip.hip launch_tiles), else 1"""
        a = C.c_uint32()
        _chk(self.L.bsgs_debug_last_tiles_per_block(self.h, C.byref(a)))
        return a.value

    def table_info(self):
        lay, nb, ov = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _chk(self.L.bsgs_table_info(self.h, C.byref(lay), C.byref(nb), C.byref(ov)))
        return lay.value, nb.value, ov.value

    def step(self, px, py, max_hits=4096):
        hits = (Hit * max_hits)()
        n = C.c_uint32()
        _chk(self.L.bsgs_step(self.h, le32(px), le32(py), hits, max_hits, C.byref(n)), allow_overflow=True)
        return [(hits[i].code, hits[i].idx) for i in range(min(n.value, max_hits))], n.value

    def run(self, centres, max_hits=65536):
        """centres: list of (x, y) ints.  Returns (hits [(tile, code, idx)], total, kernel_ms)."""
        blob = b"".join(le32(x) + le32(y) for x, y in centres)
        return self.run_raw(blob, len(centres), max_hits)

    def run_raw(self, blob, ntiles, max_hits=65536):
        hits = (HitEx * max_hits)()
        n, ms = C.c_uint32(), C.c_float()
        _chk(self.L.bsgs_run(self.h, blob, ntiles, hits, max_hits, C.byref(n), C.byref(ms)), allow_overflow=True)
        return [(hits[i].tile, hits[i].code, hits[i].idx) for i in range(min(n.value, max_hits))], n.value, ms.value

    def enqueue_raw(self, blob, ntiles):
        _chk(self.L.bsgs_enqueue(self.h, blob, ntiles))

    def collect(self, max_hits=65536):
        hits = (HitEx * max_hits)()
        n, ms = C.c_uint32(), C.c_float()
        _chk(self.L.bsgs_collect(self.h, hits, max_hits, C.byref(n), C.byref(ms)), allow_overflow=True)
        return [(hits[i].tile, hits[i].code, hits[i].idx) for i in range(min(n.value, max_hits))], n.value, ms.value

    def set_tiles_per_launch(self, n):
        _chk(self.L.bsgs_set_tiles_per_launch(self.h, n))

    def tiles_per_launch(self):
        n = C.c_uint32()
        _chk(self.L.bsgs_tiles_per_launch(self.h, C.byref(n)))
        return n.value

    def engine_geometry(self):
        a, b = C.c_uint32(), C.c_uint32()
        _chk(self.L.bsgs_engine_geometry(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_flags(self, flags):
        _chk(self.L.bsgs_set_flags(self.h, flags))

    def quirk_count(self):
        """giants of the resident G2 that reference-quirk mode re-computes (their Gy trips the reference's NEGMODP)"""
        n = C.c_uint32()
        _chk(self.L.bsgs_quirk_count(self.h, C.byref(n)))
        return n.value

    # ---- device-side tile walk: centre of tile k = P0 + k*stride, derived on the GPU ----
    def set_walk(self, p0, stride):
        _chk(self.L.bsgs_set_walk(self.h, le32(p0[0]) + le32(p0[1]), le32(stride[0]) + le32(stride[1])))

    def enqueue_walk(self, first, ntiles):
        _chk(self.L.bsgs_enqueue_walk(self.h, first, ntiles))

    def run_walk(self, first, ntiles, max_hits=65536):
        hits = (HitEx * max_hits)()
        n, ms = C.c_uint32(), C.c_float()
        _chk(self.L.bsgs_run_walk(self.h, first, ntiles, hits, max_hits, C.byref(n), C.byref(ms)), allow_overflow=True)
        return [(hits[i].tile, hits[i].code, hits[i].idx) for i in range(min(n.value, max_hits))], n.value, ms.value

    def walk_centres(self, first, ntiles):
        out = C.create_string_buffer(64 * ntiles)
        _chk(self.L.bsgs_walk_centres(self.h, first, ntiles, C.cast(out, C.c_void_p)))
        r = out.raw
        return [(int.from_bytes(r[64 * k:64 * k + 32], "little"), int.from_bytes(r[64 * k + 32:64 * k + 64], "little")) for k in range(ntiles)]

    def run_digest(self, centres, max_hits=65536):
        """like run(); also returns per (tile, engine thread) the (xor, sum) of every 64-bit key probed"""
        import numpy as np
        ntiles = len(centres)
        threads, _ = self.engine_geometry()
        blob = b"".join(le32(x) + le32(y) for x, y in centres)
        dg = np.zeros((ntiles, threads, 2), dtype=np.uint64)
        hits = (HitEx * max_hits)()
        n = C.c_uint32()
        _chk(self.L.bsgs_run_digest(self.h, blob, ntiles, dg.ctypes.data_as(C.c_void_p), hits, max_hits, C.byref(n)), allow_overflow=True)
        return dg, [(hits[i].tile, hits[i].code, hits[i].idx) for i in range(min(n.value, max_hits))], n.value

    def launch_count(self):
        n = C.c_uint64()
        _chk(self.L.bsgs_launch_count(self.h, C.byref(n)))
        return n.value

    def steps_per_tile(self):
        s = C.c_uint64()
        _chk(self.L.bsgs_steps_per_tile(self.h, C.byref(s)))
        return s.value

    def stream(self):
        s = C.c_void_p()
        _chk(self.L.bsgs_dev_stream(self.h, C.byref(s)))
        return s.value

    def selftest_fe(self, op, a_list, b_list):
        n = len(a_list)
        a = b"".join(le32(v) for v in a_list)
        b = b"".join(le32(v) for v in b_list)
        out = C.create_string_buffer(32 * n)
        _chk(self.L.bsgs_selftest_fe(self.h, op, a, b, C.cast(out, C.c_void_p), n))
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n)]

    def selftest_fe3(self, op, a_list, b_list=None, c_list=None, raw=False):
        """op (FE3_*) on every (a, b, c), any values below 2^256; raw: the result as the device function left it, not canonicalised.  The predicates give 0 or 1."""
        n = len(a_list)
        a, b, c = (b"".join(le32(v) for v in (lst if lst is not None else a_list)) for lst in (a_list, b_list, c_list))
        out = C.create_string_buffer(32 * n)
        _chk(self.L.bsgs_selftest_fe3(self.h, op, 1 if raw else 0, a, b, c, C.cast(out, C.c_void_p), n))
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n)]

    def selftest_lo64(self, a_list, b_list, iters):
        """(mismatches, exact-path cases, cases) of the low-64 squaring path vs the full-width arithmetic"""
        n = len(a_list)
        out = (C.c_uint64 * 3)()
        _chk(self.L.bsgs_selftest_lo64(self.h, b"".join(le32(v) for v in a_list), b"".join(le32(v) for v in b_list), n, iters, out))
        return int(out[0]), int(out[1]), int(out[2])

    def selftest_xs(self, px, py, first, count):
        out = C.create_string_buffer(96 * count)
        _chk(self.L.bsgs_selftest_xs(self.h, le32(px), le32(py), first, count, C.cast(out, C.c_void_p)))
        r = []
        for k in range(count):
            v = [int.from_bytes(out.raw[96 * k + 32 * i:96 * k + 32 * i + 32], "little") for i in range(3)]
            r.append((v[0], v[1], v[2] & 1))
        return r

    def profile_phases(self, blob, ntiles):
        ms = (C.c_float * 3)()
        _chk(self.L.bsgs_profile_phases(self.h, blob, ntiles, ms))
        return [float(x) for x in ms]

    def bench_random_read(self, footprint_bytes, granule=64):
        g, r = C.c_double(), C.c_double()
        _chk(self.L.bsgs_bench_random_read(self.h, footprint_bytes, granule, C.byref(g), C.byref(r)))
        return g.value, r.value

    def bench_stream(self, kind, nbytes):
        """GB/s of one pass over nbytes in a streaming pattern of the tile kernel (0 coalesced loads, 1 the same by LDS-DMA, 2 non-temporal stores)"""
        g = C.c_double()
        _chk(self.L.bsgs_bench_stream(self.h, kind, nbytes, C.byref(g)))
        return g.value

    def debug_buffers(self, measure=True):
        a = (C.c_uint64 * 5)()
        g = C.c_double()
        _chk(self.L.bsgs_debug_buffers(self.h, a, C.byref(g) if measure else None))
        return [int(x) for x in a], g.value

    def xcd_profile(self, first, ntiles):
        """([(ms until XCD x finished its last block, blocks it ran)] x 8, launch ms)"""
        out = (C.c_uint64 * 16)()
        ms = C.c_float()
        _chk(self.L.bsgs_debug_xcd_profile(self.h, first, ntiles, out, C.byref(ms)))
        return [(out[2 * x] / 1e5, int(out[2 * x + 1])) for x in range(8)], ms.value

    def chain_placement(self):
        """how the chain scratch was placed (bsgs_chain_placement)"""
        info, grade = (C.c_uint32 * 5)(), (C.c_float * 2)()
        self.L.bsgs_chain_placement.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        _chk(self.L.bsgs_chain_placement(self.h, info, grade))
        g, n, sep = (C.c_float * 64)(), C.c_uint32(), C.c_uint32()
        self.L.bsgs_chain_grades.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _chk(self.L.bsgs_chain_grades(self.h, g, 64, C.byref(n), C.byref(sep)))
        return {"pieces": int(info[0]), "tiles_per_piece": int(info[1]), "graded": int(info[2]), "handed_back": int(info[3]),
                "from_reserved_group": bool(info[4]), "best_grade_G_per_s": round(grade[0], 2), "worst_kept_grade_G_per_s": round(grade[1], 2),
                "separation_seen": bool(sep.value) or bool(info[4]), "grades_kept_first": [round(g[k], 1) for k in range(min(n.value, 64))]}

    def tune_placement(self, candidates=3):
        """start-up tuning of where chain scratch and bucket lines lie (bsgs_tune_placement):
        {"chain_ms": [...], "lines_ms": [...], "kept": (i, j), "final_ms": ms}"""
        ms = (C.c_float * (2 * candidates))()
        chosen = (C.c_uint32 * 2)()
        fin = C.c_float()
        self.L.bsgs_tune_placement.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        _chk(self.L.bsgs_tune_placement(self.h, candidates, ms, chosen, C.byref(fin)))
        return {"chain_ms": [round(ms[k], 2) for k in range(candidates) if ms[k] > 0], "lines_ms": [round(ms[candidates + k], 2) for k in range(candidates) if ms[candidates + k] > 0],
                "kept": (int(chosen[0]), int(chosen[1])), "final_ms": round(fin.value, 2)}

    def debug_realloc(self, which, spacer_bytes=0):
        _chk(self._test_hook("bsgs_debug_realloc")(self.h, which, spacer_bytes))

    def bench_modmul(self):
        g = C.c_double()
        _chk(self.L.bsgs_bench_modmul(self.h, C.byref(g)))
        return g.value

    # ---- kangaroo walk (include/bsgs_hip.h "Kangaroo"): states are (x, y, d, flags) with d an integer mod 2^128 (two's complement), records dicts
    def kangaroo_setup(self, jumps, scalars, dp, herd, per_thread, record_cap):
        """jumps = 64 affine points (x, y), scalars = their s_j; herd kangaroos, per_thread of them per GPU thread; record_cap records per launch"""
        if len(jumps) != KANGAROO_JUMPS or len(scalars) != KANGAROO_JUMPS:
            raise BsgsError("kangaroo_setup: %d jump points and scalars" % KANGAROO_JUMPS)
        xy = b"".join(le32(x) + le32(y) for x, y in jumps)
        _chk(self.L.bsgs_kangaroo_setup(self.h, xy, (C.c_uint64 * KANGAROO_JUMPS)(*scalars), dp, herd, per_thread, record_cap))
        self._kang_cap, self._kang_keyed = record_cap, False

    def kangaroo_setup_sym(self, jumps, scalars, dp, herd, per_thread, record_cap):
        """the symmetric walk (negation map): len(jumps) = R affine points, a power of two in 64..4096; the other kangaroo_* calls then run that walk"""
        if len(jumps) != len(scalars):
            raise BsgsError("kangaroo_setup_sym: as many scalars as jump points")
        xy = b"".join(le32(x) + le32(y) for x, y in jumps)
        _chk(self.L.bsgs_kangaroo_setup_sym(self.h, xy, (C.c_uint64 * len(scalars))(*scalars), len(jumps), dp, herd, per_thread, record_cap))
        self._kang_cap, self._kang_keyed = record_cap, False

    def kangaroo_setup_sym_keys(self, jumps, scalars, dp, herd, per_thread, record_cap):
        """the symmetric walk for a key list: as kangaroo_setup_sym plus a key per kangaroo.  States of this herd are (x, y, d, flags, key) both ways, and
        every record's "key" names the key of its kangaroo; kangaroo_set_keys / kangaroo_seed_keys serve it (stored flags: KANGAROO_WILD, no key bits)"""
        if len(jumps) != len(scalars):
            raise BsgsError("kangaroo_setup_sym_keys: as many scalars as jump points")
        xy = b"".join(le32(x) + le32(y) for x, y in jumps)
        _chk(self.L.bsgs_kangaroo_setup_sym_keys(self.h, xy, (C.c_uint64 * len(scalars))(*scalars), len(jumps), dp, herd, per_thread, record_cap))
        self._kang_cap, self._kang_keyed = record_cap, True

    @staticmethod
    def _kangaroo_states(states):
        arr = (KangarooState * len(states))()
        for k, (x, y, d, fl, *key) in enumerate(states):
            arr[k].x[:] = le32(x)
            arr[k].y[:] = le32(y)
            arr[k].d[:] = (d % (1 << 128)).to_bytes(16, "little")
            arr[k].flags = fl
            if key:                                                # (x, y, d, flags, key): a herd of kangaroo_setup_sym_keys; others ignore the word
                arr[k].reserved[0] = key[0]
        return arr

    def kangaroo_upload(self, first, states):
        _chk(self.L.bsgs_kangaroo_upload(self.h, first, len(states), self._kangaroo_states(states)))

    def kangaroo_upload_list(self, idx, states):
        assert len(idx) == len(states)
        _chk(self.L.bsgs_kangaroo_upload_list(self.h, (C.c_uint32 * len(idx))(*idx), len(idx), self._kangaroo_states(states)))

    def kangaroo_download(self, first, n, reserved=False):
        """states (x, y, d, flags), of a herd of kangaroo_setup_sym_keys (x, y, d, flags, key); reserved=True: every state followed by the three reserved
        words of bsgs_kangaroo_state as a tuple, whatever the herd"""
        arr = (KangarooState * n)()
        _chk(self.L.bsgs_kangaroo_download(self.h, first, n, arr))
        keyed = self._kang_keyed
        return [(int.from_bytes(bytes(s.x), "little"), int.from_bytes(bytes(s.y), "little"), int.from_bytes(bytes(s.d), "little"), s.flags) +
                ((s.reserved[0],) if keyed else ()) + ((tuple(s.reserved),) if reserved else ()) for s in arr]

    # raw=True on the calls below: records cross as the bytes of 64-byte bsgs_kangaroo_record, without one Python object per record
    @staticmethod
    def _raw_records_in(records):
        """the bytes of m records (anything with the buffer protocol) -> (a pointer the C-ABI takes, m, the object that keeps the bytes alive)"""
        b = records if isinstance(records, bytes) else bytes(records)
        if len(b) % 64:
            raise BsgsError("raw records: %d bytes are no multiple of 64" % len(b))
        return C.cast(C.c_char_p(b), C.POINTER(KangarooRecord)), len(b) // 64, b

    @staticmethod
    def _raw_records_out(cap):
        buf = C.create_string_buffer(64 * max(1, cap))
        return C.cast(buf, C.POINTER(KangarooRecord)), buf

    def kangaroo_run(self, steps, raw=False):
        """one launch of `steps` steps: (records, dropped, kernel ms); a record is {x, d (mod 2^128), kangaroo, flags, step, key}, key = the key of
        the kangaroo in a herd of kangaroo_setup_sym_keys and 0 in every other; raw: the bytes of the records in the place of the list"""
        cap = self._kang_cap
        n, dropped, ms = C.c_uint32(), C.c_uint64(), C.c_float()
        if raw:
            recs, buf = self._raw_records_out(cap)
            _chk(self.L.bsgs_kangaroo_run(self.h, steps, recs, cap, C.byref(n), C.byref(dropped), C.byref(ms)))
            return buf.raw[:64 * n.value], dropped.value, ms.value
        recs = (KangarooRecord * cap)()
        _chk(self.L.bsgs_kangaroo_run(self.h, steps, recs, cap, C.byref(n), C.byref(dropped), C.byref(ms)))
        out = [{"x": int.from_bytes(bytes(r.x), "little"), "d": int.from_bytes(bytes(r.d), "little"), "kangaroo": r.kangaroo, "flags": r.flags, "step": r.step, "key": r.reserved}
               for r in recs[:n.value]]
        return out, dropped.value, ms.value

    def kangaroo_tames_install(self, tags):
        """the tame table of the herd: tags = the low 64 bits of x of its entries, pairwise different, in entry order; replaces an earlier table and lives
        as long as the herd (kangaroo_setup, kangaroo_setup_sym)"""
        _chk(self.L.bsgs_kangaroo_tames_install(self.h, (C.c_uint64 * max(1, len(tags)))(*tags), len(tags)))

    def kangaroo_run_tames(self, steps, raw=False):
        """one launch of `steps` steps matched against the tame table on the device: (records, n_seen, dropped, kernel ms).  Only the records whose x is in
        the table and the DEAD ones come back, as kangaroo_run's plus "entry": the table entry's number, None for a DEAD record that matched nothing;
        n_seen = the records the walk produced; raw: the bytes of the records (`reserved` = entry number + 1, 0 for None) in the place of the list"""
        cap = max(1, self._kang_cap)
        n, seen, dropped, ms = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_float()
        if raw:
            recs, buf = self._raw_records_out(cap)
            _chk(self.L.bsgs_kangaroo_run_tames(self.h, steps, recs, cap, C.byref(n), C.byref(seen), C.byref(dropped), C.byref(ms)))
            return buf.raw[:64 * n.value], seen.value, dropped.value, ms.value
        recs = (KangarooRecord * cap)()
        _chk(self.L.bsgs_kangaroo_run_tames(self.h, steps, recs, cap, C.byref(n), C.byref(seen), C.byref(dropped), C.byref(ms)))
        out = [{"x": int.from_bytes(bytes(r.x), "little"), "d": int.from_bytes(bytes(r.d), "little"), "kangaroo": r.kangaroo, "flags": r.flags, "step": r.step,
                "entry": r.reserved - 1 if r.reserved else None} for r in recs[:n.value]]
        return out, seen.value, dropped.value, ms.value

    def kangaroo_tames_install_keys(self, tags):
        """kangaroo_tames_install for the herd of kangaroo_setup_sym_keys, whose records keep their key"""
        _chk(self.L.bsgs_kangaroo_tames_install_keys(self.h, (C.c_uint64 * max(1, len(tags)))(*tags), len(tags)))

    def kangaroo_run_tames_keys(self, steps, max_recs=None, raw=False):
        """kangaroo_run_tames for the herd of kangaroo_setup_sym_keys: every record also has "key" (the word the walk wrote), and "entry" comes from the
        parallel array (entry number, None for a DEAD record that matched nothing); max_recs: a host buffer smaller than the record capacity; raw: (the
        bytes of the records, the bytes of their u32 entry words: entry number + 1, 0 for None) in the place of the list"""
        cap = max(1, self._kang_cap if max_recs is None else max_recs)
        n, seen, dropped, ms = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_float()
        if raw:
            recs, buf = self._raw_records_out(cap)
            ent = (C.c_uint32 * cap)()
            _chk(self.L.bsgs_kangaroo_run_tames_keys(self.h, steps, recs, ent, cap, C.byref(n), C.byref(seen), C.byref(dropped), C.byref(ms)))
            return (buf.raw[:64 * n.value], bytes(ent)[:4 * n.value]), seen.value, dropped.value, ms.value
        recs, ent = (KangarooRecord * cap)(), (C.c_uint32 * cap)()
        _chk(self.L.bsgs_kangaroo_run_tames_keys(self.h, steps, recs, ent, cap, C.byref(n), C.byref(seen), C.byref(dropped), C.byref(ms)))
        out = [{"x": int.from_bytes(bytes(r.x), "little"), "d": int.from_bytes(bytes(r.d), "little"), "kangaroo": r.kangaroo, "flags": r.flags, "step": r.step,
                "key": r.reserved, "entry": e - 1 if e else None} for r, e in zip(recs[:n.value], ent[:n.value])]
        return out, seen.value, dropped.value, ms.value

    # ---- the tame table grown on the device (include/bsgs_hip.h "Kangaroo, tame table grown on the device")
    def kangaroo_tames_gen_begin(self, capacity):
        """allocates the growing table for `capacity` entries under the herd of kangaroo_setup / kangaroo_setup_sym; replaces an earlier one"""
        _chk(self.L.bsgs_kangaroo_tames_gen_begin(self.h, capacity))

    @staticmethod
    def _gen_handed_back(recs, n):
        return [{"x": int.from_bytes(bytes(r.x), "little"), "d": int.from_bytes(bytes(r.d), "little"), "kangaroo": r.kangaroo, "flags": r.flags, "step": r.step,
                 "reason": r.reserved} for r in recs[:n]]

    def kangaroo_run_tames_gen(self, steps, max_recs=None, raw=False):
        """one launch of `steps` steps inserted into the growing table on the device: (handed-back records, n_seen, n_entries, dropped, kernel ms); a
        handed-back record is kangaroo_run's with "reason" (KANGAROO_GEN_*) in the place of "key"; raw: their bytes (the reason in `reserved`) """
        cap = max(1, self._kang_cap if max_recs is None else max_recs)
        n, seen, entries, dropped, ms = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        if raw:
            recs, buf = self._raw_records_out(cap)
            _chk(self.L.bsgs_kangaroo_run_tames_gen(self.h, steps, recs, cap, C.byref(n), C.byref(seen), C.byref(entries), C.byref(dropped), C.byref(ms)))
            return buf.raw[:64 * n.value], seen.value, entries.value, dropped.value, ms.value
        recs = (KangarooRecord * cap)()
        _chk(self.L.bsgs_kangaroo_run_tames_gen(self.h, steps, recs, cap, C.byref(n), C.byref(seen), C.byref(entries), C.byref(dropped), C.byref(ms)))
        return self._gen_handed_back(recs, n.value), seen.value, entries.value, dropped.value, ms.value

    def kangaroo_tames_gen_insert(self, records, raw=False):
        """the insert alone on records of the caller's, (tag or x, d, flags[, kangaroo]) each: (handed-back records, n_entries); raw: records = the bytes
        of 64-byte records, inserted as they are, and the handed-back ones come as bytes too (the reason in `reserved`)"""
        if raw:
            arr, m, keep = self._raw_records_in(records)
            cap = max(1, self._kang_cap)
            out, buf = self._raw_records_out(cap)
            n, entries = C.c_uint32(), C.c_uint64()
            _chk(self.L.bsgs_kangaroo_tames_gen_insert(self.h, arr, m, out, cap, C.byref(n), C.byref(entries)))
            return buf.raw[:64 * n.value], entries.value
        m = len(records)
        arr = (KangarooRecord * max(1, m))()
        for k, (x, d, fl, *kang) in enumerate(records):
            arr[k].x[:] = le32(x)
            arr[k].d[:] = (d % (1 << 128)).to_bytes(16, "little")
            arr[k].flags = fl
            arr[k].kangaroo = kang[0] if kang else k
        cap = max(1, self._kang_cap)
        out = (KangarooRecord * cap)()
        n, entries = C.c_uint32(), C.c_uint64()
        _chk(self.L.bsgs_kangaroo_tames_gen_insert(self.h, arr, m, out, cap, C.byref(n), C.byref(entries)))
        return self._gen_handed_back(out, n.value), entries.value

    def kangaroo_tames_gen_read(self, max_entries=None, raw=False):
        """the table's entries as a list of (tag, d mod 2^128), in any order; max_entries: the room offered (None: what the table holds); raw: (the tags
        as the bytes of little-endian u64, the offsets as bytes) in the place of the list"""
        n = C.c_uint64()
        if max_entries is None:
            rc = self.L.bsgs_kangaroo_tames_gen_read(self.h, None, None, 0, C.byref(n))
            if n.value == 0:
                _chk(rc)
                return (b"", b"") if raw else []
            max_entries = n.value
        tags, d = (C.c_uint64 * max(1, max_entries))(), C.create_string_buffer(16 * max(1, max_entries))
        _chk(self.L.bsgs_kangaroo_tames_gen_read(self.h, tags, d, max_entries, C.byref(n)))
        db = d.raw
        if raw:
            return bytes(tags)[:8 * n.value], db[:16 * n.value]
        return [(tags[k], int.from_bytes(db[16 * k:16 * k + 16], "little")) for k in range(n.value)]

    def kangaroo_tames_gen_end(self):
        _chk(self.L.bsgs_kangaroo_tames_gen_end(self.h))

    def kangaroo_tames_gen_load(self, tags, d):
        """n (tag, d) pairs into the growing table, 24 bytes each: tags = n integers or the bytes of n little-endian u64, d = n integers (taken mod 2^128) or
        the bytes of n 16-byte offsets -> (stored, duplicate, zero, full, n_entries)"""
        tb = bytes(tags) if isinstance(tags, (bytes, bytearray, memoryview)) else b"".join(t.to_bytes(8, "little") for t in tags)
        db = bytes(d) if isinstance(d, (bytes, bytearray, memoryview)) else b"".join((v % (1 << 128)).to_bytes(16, "little") for v in d)
        n = len(tb) // 8
        assert len(tb) == 8 * n and len(db) == 16 * n
        out = [C.c_uint64() for _ in range(5)]
        _chk(self.L.bsgs_kangaroo_tames_gen_load(self.h, C.c_char_p(tb), C.c_char_p(db), n, *[C.byref(v) for v in out]))
        return tuple(v.value for v in out)

    def kangaroo_tames_gen_read_sorted(self, max_entries=None, raw=False):
        """the table's entries ascending by tag, sorted on the device, cut to the max_entries lowest tags (None: all of them): (list of (tag, d mod 2^128), the
        table's entry count); raw: the tags and the offsets as bytes in the place of the list"""
        n = C.c_uint64()
        _chk(self.L.bsgs_kangaroo_tames_gen_read_sorted(self.h, None, None, 0, C.byref(n)))
        m = n.value if max_entries is None else max_entries
        tags, d = C.create_string_buffer(8 * max(1, m)), C.create_string_buffer(16 * max(1, m))
        _chk(self.L.bsgs_kangaroo_tames_gen_read_sorted(self.h, tags, d, m, C.byref(n)))
        got = min(m, n.value)
        tb, db = tags.raw[:8 * got], d.raw[:16 * got]
        if raw:
            return (tb, db), n.value
        return [(int.from_bytes(tb[8 * k:8 * k + 8], "little"), int.from_bytes(db[16 * k:16 * k + 16], "little")) for k in range(got)], n.value

    # ---- the distinguished-point table in device memory (include/bsgs_hip.h "Kangaroo, distinguished-point table in device memory")
    def kangaroo_dptable_begin(self, capacity):
        """allocates the table for `capacity` entries under the herd of kangaroo_setup / kangaroo_setup_sym; replaces an earlier one"""
        _chk(self.L.bsgs_kangaroo_dptable_begin(self.h, capacity))

    def kangaroo_run_dptable(self, steps, max_recs=None, raw=False):
        """one launch of `steps` steps inserted into the table on the device: (hand-backs, n_seen, n_entries, dropped, kernel ms); a hand-back is
        kangaroo_run's record with "reason" (KANGAROO_DPT_*) in the place of "key", and a duplicate is two of them: the stored entry (reason
        KANGAROO_DPT_STORED, x = its tag, flags = its type), then the walk's record; max_recs: a host buffer of another size than two per record; raw: the
        bytes of the hand-backs (the reason in `reserved`) in the place of the list"""
        cap = 2 * self._kang_cap if max_recs is None else max_recs
        n, seen, entries, dropped, ms = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        if raw:
            recs, buf = self._raw_records_out(cap)
            _chk(self.L.bsgs_kangaroo_run_dptable(self.h, steps, recs, cap, C.byref(n), C.byref(seen), C.byref(entries), C.byref(dropped), C.byref(ms)))
            return buf.raw[:64 * n.value], seen.value, entries.value, dropped.value, ms.value
        recs = (KangarooRecord * max(1, cap))()
        _chk(self.L.bsgs_kangaroo_run_dptable(self.h, steps, recs, cap, C.byref(n), C.byref(seen), C.byref(entries), C.byref(dropped), C.byref(ms)))
        return self._gen_handed_back(recs, n.value), seen.value, entries.value, dropped.value, ms.value

    def kangaroo_dptable_insert(self, records, max_recs=None, raw=False):
        """insert and resolve alone on records of the caller's, (tag or x, d, flags[, kangaroo]) each: (hand-backs, n_entries, dropped); raw: records = the
        bytes of 64-byte records, inserted as they are, and the hand-backs come as bytes too (the reason in `reserved`)"""
        if raw:
            arr, m, keep = self._raw_records_in(records)
            cap = 2 * self._kang_cap if max_recs is None else max_recs
            out, buf = self._raw_records_out(cap)
            n, entries, dropped = C.c_uint32(), C.c_uint64(), C.c_uint64()
            _chk(self.L.bsgs_kangaroo_dptable_insert(self.h, arr, m, out, cap, C.byref(n), C.byref(entries), C.byref(dropped)))
            return buf.raw[:64 * n.value], entries.value, dropped.value
        m = len(records)
        arr = (KangarooRecord * max(1, m))()
        for k, (x, d, fl, *kang) in enumerate(records):
            arr[k].x[:] = le32(x)
            arr[k].d[:] = (d % (1 << 128)).to_bytes(16, "little")
            arr[k].flags = fl
            arr[k].kangaroo = kang[0] if kang else k
        cap = 2 * self._kang_cap if max_recs is None else max_recs
        out = (KangarooRecord * max(1, cap))()
        n, entries, dropped = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _chk(self.L.bsgs_kangaroo_dptable_insert(self.h, arr, m, out, cap, C.byref(n), C.byref(entries), C.byref(dropped)))
        return self._gen_handed_back(out, n.value), entries.value, dropped.value

    def kangaroo_dptable_load(self, entries):
        """entries (tag, d mod 2^128, kangaroo, type), or the bytes of n 32-byte entries, into the table -> (stored, duplicate, zero, full, n_entries)"""
        raw = bytes(entries) if isinstance(entries, (bytes, bytearray, memoryview)) else b"".join(
            t.to_bytes(8, "little") + (d % (1 << 128)).to_bytes(16, "little") + k.to_bytes(4, "little") + ty.to_bytes(4, "little") for t, d, k, ty in entries)
        n = len(raw) // 32
        assert len(raw) == 32 * n
        out = [C.c_uint64() for _ in range(5)]
        _chk(self.L.bsgs_kangaroo_dptable_load(self.h, C.c_char_p(raw), n, *[C.byref(v) for v in out]))
        return tuple(v.value for v in out)

    def kangaroo_dptable_read(self, max_entries=None, raw=False):
        """the table's entries as a list of (tag, d mod 2^128, kangaroo, type), in any order; max_entries: the room offered (None: what the table holds);
        raw: the bytes of the 32-byte entries in the place of the list"""
        n = C.c_uint64()
        if max_entries is None:
            rc = self.L.bsgs_kangaroo_dptable_read(self.h, None, 0, C.byref(n))
            if n.value == 0:
                _chk(rc)
                return b"" if raw else []
            max_entries = n.value
        buf = C.create_string_buffer(32 * max(1, max_entries))
        _chk(self.L.bsgs_kangaroo_dptable_read(self.h, buf, max_entries, C.byref(n)))
        b = buf.raw[:32 * n.value]
        if raw:
            return b
        return [(int.from_bytes(b[o:o + 8], "little"), int.from_bytes(b[o + 8:o + 24], "little"), int.from_bytes(b[o + 24:o + 28], "little"),
                 int.from_bytes(b[o + 28:o + 32], "little")) for o in range(0, len(b), 32)]

    def kangaroo_dptable_end(self):
        _chk(self.L.bsgs_kangaroo_dptable_end(self.h))

    # ---- the distinguished-point table for a key list (include/bsgs_hip.h "Kangaroo, distinguished-point table for a key list")
    @staticmethod
    def _keys_handed_back(recs, n):
        """a hand-back of the keyed table: the stored half of a pair has reason KANGAROO_DPT_STORED, flags = its owner word and key None; a record of the
        walk has its reason and the key it named"""
        out = []
        for r in recs[:n]:
            stored = r.reserved == KANGAROO_DPT_STORED
            out.append({"x": int.from_bytes(bytes(r.x), "little"), "d": int.from_bytes(bytes(r.d), "little"), "kangaroo": r.kangaroo, "flags": r.flags, "step": r.step,
                        "reason": KANGAROO_DPT_STORED if stored else r.reserved & ((1 << KANGAROO_DPT_KEY_SHIFT) - 1),
                        "key": None if stored else r.reserved >> KANGAROO_DPT_KEY_SHIFT})
        return out

    def kangaroo_dptable_begin_keys(self, capacity):
        """allocates the keyed table for `capacity` entries under a herd of kangaroo_setup / kangaroo_setup_sym_keys that has a key list"""
        _chk(self.L.bsgs_kangaroo_dptable_begin_keys(self.h, capacity))

    def kangaroo_run_dptable_keys(self, steps, max_recs=None, raw=False):
        """kangaroo_run_dptable on the keyed table: (hand-backs, n_seen, n_entries, dropped, kernel ms); a hand-back has "reason" and "key"; raw: the bytes
        of the hand-backs (`reserved` = reason | key << KANGAROO_DPT_KEY_SHIFT)"""
        cap = 2 * self._kang_cap if max_recs is None else max_recs
        n, seen, entries, dropped, ms = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        if raw:
            recs, buf = self._raw_records_out(cap)
            _chk(self.L.bsgs_kangaroo_run_dptable_keys(self.h, steps, recs, cap, C.byref(n), C.byref(seen), C.byref(entries), C.byref(dropped), C.byref(ms)))
            return buf.raw[:64 * n.value], seen.value, entries.value, dropped.value, ms.value
        recs = (KangarooRecord * max(1, cap))()
        _chk(self.L.bsgs_kangaroo_run_dptable_keys(self.h, steps, recs, cap, C.byref(n), C.byref(seen), C.byref(entries), C.byref(dropped), C.byref(ms)))
        return self._keys_handed_back(recs, n.value), seen.value, entries.value, dropped.value, ms.value

    def kangaroo_dptable_insert_keys(self, records, max_recs=None, raw=False):
        """the keyed insert and the resolve alone on records of the caller's, (tag or x, d, flags, kangaroo, reserved) each: (hand-backs, n_entries,
        dropped); raw: records = the bytes of 64-byte records, and the hand-backs come as bytes too"""
        cap = 2 * self._kang_cap if max_recs is None else max_recs
        n, entries, dropped = C.c_uint32(), C.c_uint64(), C.c_uint64()
        if raw:
            arr, m, keep = self._raw_records_in(records)
            out, buf = self._raw_records_out(cap)
            _chk(self.L.bsgs_kangaroo_dptable_insert_keys(self.h, arr, m, out, cap, C.byref(n), C.byref(entries), C.byref(dropped)))
            return buf.raw[:64 * n.value], entries.value, dropped.value
        m = len(records)
        arr = (KangarooRecord * max(1, m))()
        for k, (x, d, fl, kang, res) in enumerate(records):
            arr[k].x[:] = le32(x)
            arr[k].d[:] = (d % (1 << 128)).to_bytes(16, "little")
            arr[k].flags, arr[k].kangaroo, arr[k].reserved = fl, kang, res
        out = (KangarooRecord * max(1, cap))()
        _chk(self.L.bsgs_kangaroo_dptable_insert_keys(self.h, arr, m, out, cap, C.byref(n), C.byref(entries), C.byref(dropped)))
        return self._keys_handed_back(out, n.value), entries.value, dropped.value

    # ---- the distinguished-point table divided over engines (include/bsgs_hip.h "Kangaroo, distinguished-point table divided over engines")
    def kangaroo_dptable_begin_shard(self, capacity, shard, shards, kangaroo_base=0):
        """allocates shard `shard` of a table of `shards` shards, `capacity` entries here, under the herd of kangaroo_setup / kangaroo_setup_sym; the herd's
        kangaroos are kangaroo_base + index wherever a record leaves the device"""
        _chk(self.L.bsgs_kangaroo_dptable_begin_shard(self.h, capacity, shard, shards, kangaroo_base))
        self._dpt_shards = shards

    def _routed_groups(self, recs, buf, counts, raw):
        """the routed records as one group per shard, in the shards' order: bytes (raw) or hand-back style records with `reserved` as "reason" """
        out, at = [], 0
        for c in counts:
            out.append(buf.raw[64 * at:64 * (at + c)] if raw else self._gen_handed_back(recs[at:at + c], c))
            at += c
        return out

    def kangaroo_run_dptable_shard(self, steps, max_recs=None, max_routed=None, raw=False):
        """kangaroo_run_dptable on a sharded table: (hand-backs, routed, n_seen, n_entries, dropped, kernel ms); routed = one group of records per shard
        (the own shard's empty), every id global; raw: bytes in the place of the lists"""
        cap = 2 * self._kang_cap if max_recs is None else max_recs
        rcap = self._kang_cap if max_routed is None else max_routed
        n, seen, entries, dropped, ms = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        counts = (C.c_uint32 * KANGAROO_DPT_MAX_SHARDS)()
        recs, buf = self._raw_records_out(cap)
        routed, rbuf = self._raw_records_out(rcap)
        _chk(self.L.bsgs_kangaroo_run_dptable_shard(self.h, steps, recs, cap, C.byref(n), routed, rcap, counts, C.byref(seen), C.byref(entries), C.byref(dropped),
                                                    C.byref(ms)))
        groups = self._routed_groups(routed, rbuf, list(counts)[:self._dpt_shards], raw)
        return (buf.raw[:64 * n.value] if raw else self._gen_handed_back(recs, n.value)), groups, seen.value, entries.value, dropped.value, ms.value

    def kangaroo_dptable_insert_shard(self, records, max_recs=None, max_routed=None, raw=False):
        """insert with routing and resolve alone on records of the caller's, (tag or x, d, flags, kangaroo) each, their ids global: (hand-backs, routed,
        n_entries, dropped); raw: records = the bytes of 64-byte records, and bytes come back"""
        if raw:
            arr, m, keep = self._raw_records_in(records)
        else:
            m = len(records)
            arr = (KangarooRecord * max(1, m))()
            for k, (x, d, fl, kang) in enumerate(records):
                arr[k].x[:] = le32(x)
                arr[k].d[:] = (d % (1 << 128)).to_bytes(16, "little")
                arr[k].flags, arr[k].kangaroo = fl, kang
        cap = 2 * self._kang_cap if max_recs is None else max_recs
        rcap = self._kang_cap if max_routed is None else max_routed
        n, entries, dropped = C.c_uint32(), C.c_uint64(), C.c_uint64()
        counts = (C.c_uint32 * KANGAROO_DPT_MAX_SHARDS)()
        out, buf = self._raw_records_out(cap)
        routed, rbuf = self._raw_records_out(rcap)
        _chk(self.L.bsgs_kangaroo_dptable_insert_shard(self.h, arr, m, out, cap, C.byref(n), routed, rcap, counts, C.byref(entries), C.byref(dropped)))
        groups = self._routed_groups(routed, rbuf, list(counts)[:self._dpt_shards], raw)
        return (buf.raw[:64 * n.value] if raw else self._gen_handed_back(out, n.value)), groups, entries.value, dropped.value

    def kangaroo_seed(self, Q, offsets, flags, first=0, idx=None):
        """start points on the GPU: kangaroo idx[k] (first + k without idx) := (d*G or Q + d*G, d, flags[k]) for d = offsets[k] (a signed integer) and
        flags[k] = 0 or KANGAROO_WILD; Q = (x, y) or None when no entry is wild.  -> (starts at infinity, lowest position of one)"""
        n = len(offsets)
        assert len(flags) == n and (idx is None or len(idx) == n)
        d = b"".join((v % (1 << 128)).to_bytes(16, "little") for v in offsets)
        q = le32(Q[0]) + le32(Q[1]) if Q is not None else None
        ninf, first_inf = C.c_uint32(), C.c_uint32()
        _chk(self.L.bsgs_kangaroo_seed(self.h, q, (C.c_uint32 * n)(*idx) if idx is not None else None, first, n, d, (C.c_uint32 * n)(*flags), C.byref(ninf),
                                       C.byref(first_inf)))
        return ninf.value, first_inf.value

    def kangaroo_set_keys(self, Qs):
        """the key list of the herd: affine points Q_k = (x, y), 1..KANGAROO_MAX_KEYS of them; replaces an earlier list"""
        _chk(self.L.bsgs_kangaroo_set_keys(self.h, b"".join(le32(x) + le32(y) for x, y in Qs), len(Qs)))

    def kangaroo_seed_keys(self, offsets, flags, keys, first=0, idx=None):
        """as kangaroo_seed with one Q per position: a wild position k starts at Q_keys[k] + d*G with flags KANGAROO_WILD | keys[k] << KANGAROO_KEY_SHIFT; a
        tame one has keys[k] == 0.  -> (starts at infinity, lowest position of one)"""
        n = len(offsets)
        assert len(flags) == n and len(keys) == n and (idx is None or len(idx) == n)
        d = b"".join((v % (1 << 128)).to_bytes(16, "little") for v in offsets)
        ninf, first_inf = C.c_uint32(), C.c_uint32()
        _chk(self.L.bsgs_kangaroo_seed_keys(self.h, (C.c_uint32 * n)(*idx) if idx is not None else None, first, n, d, (C.c_uint32 * n)(*flags),
                                            (C.c_uint32 * n)(*keys), C.byref(ninf), C.byref(first_inf)))
        return ninf.value, first_inf.value

    def kangaroo_verify(self, q=None, first=0, n=None, max_bad=64):
        """every kangaroo of [first, first + n) (n None: to the end of the herd) against sigma*Q + d*G on the GPU, the herd untouched; q = (x, y), or None:
        the list of kangaroo_set_keys.  -> (how many fail, [at most max_bad of them, ascending])"""
        if n is None:
            t, g, _ = self.kangaroo_geometry()
            n = t * g - first
        nbad, idx = C.c_uint32(), (C.c_uint32 * max(1, max_bad))()
        _chk(self.L.bsgs_kangaroo_verify(self.h, le32(q[0]) + le32(q[1]) if q is not None else None, first, n, C.byref(nbad), idx, max_bad))
        return nbad.value, list(idx[:min(nbad.value, max_bad)])

    def kangaroo_verify_points(self, q, offsets, flags, x_lo64, max_bad=64):
        """entries (d = offsets[k], a signed integer; flags[k] as a state's: WILD, NEG, key bits) against x_lo64[k], the low 64 bits of x(sigma*Q + d*G);
        needs a herd (kangaroo_setup).  -> (how many fail, [at most max_bad positions, ascending])"""
        n = len(offsets)
        assert len(flags) == n and len(x_lo64) == n
        d = b"".join((v % (1 << 128)).to_bytes(16, "little") for v in offsets)
        nbad, idx = C.c_uint32(), (C.c_uint32 * max(1, max_bad))()
        _chk(self.L.bsgs_kangaroo_verify_points(self.h, le32(q[0]) + le32(q[1]) if q is not None else None, n, d, (C.c_uint32 * max(1, n))(*flags),
                                                (C.c_uint64 * max(1, n))(*x_lo64), C.byref(nbad), idx, max_bad))
        return nbad.value, list(idx[:min(nbad.value, max_bad)])

    def kangaroo_geometry(self):
        t, g, b = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _chk(self.L.bsgs_kangaroo_geometry(self.h, C.byref(t), C.byref(g), C.byref(b)))
        return t.value, g.value, b.value
