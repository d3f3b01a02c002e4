"""ctypes binding of liblime_hip.so, derived from the C ABI's one statement: include/lime_hip.h.

Nothing of the header is written out here a second time: the signatures, the argument structs and the constants below are what
_header.Header reads from it, so a new or widened entry point is an edit of the header (and of its caller in ops.py) only.

There is deliberately no fallback: if the shared library is missing or does not export a symbol,
loading raises -- the product path never routes around the HIP kernels.
"""
import ctypes
import os

from ._header import Header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'liblime_hip.so')
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'lime_hip.h')


class LimeHipError(RuntimeError):
    pass


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise LimeHipError('%s is missing: the binding of liblime_hip.so is derived from it; there is no second copy of the ABI'
                           % os.path.normpath(HEADER_PATH))
    with open(HEADER_PATH) as f:
        return Header(f.read(), 'include/lime_hip.h')


_abi = _read_header()
SIGNATURES = _abi.signatures         # name -> (restype, argtypes); every symbol include/lime_hip.h declares
STRUCTS = _abi.structs               # C name -> ctypes.Structure
CONSTANTS = _abi.constants           # enumerator / integer #define -> value
C_TYPES = _abi.c_types               # name -> (return type, parameter types) in the header's spelling

LinearArgs = STRUCTS['lime_linear_args']
LinearPlan = STRUCTS['lime_linear_plan']
LinearBf16Args = STRUCTS['lime_linear_bf16_args']
TokenAttentionArgs = STRUCTS['lime_token_attention_args']
TokenAttentionPlan = STRUCTS['lime_token_attention_plan']
TokenAttentionBwdArgs = STRUCTS['lime_token_attention_bwd_args']
TokenAttentionBwdPlan = STRUCTS['lime_token_attention_bwd_plan']
FfnBf16Args = STRUCTS['lime_ffn_bf16_args']
FfnSpArgs = STRUCTS['lime_ffn_sp_args']
OprojSpArgs = STRUCTS['lime_oproj_sp_args']
EncoderBlockBf16Args = STRUCTS['lime_encoder_block_bf16_args']
InprojBf16Args = STRUCTS['lime_inproj_bf16_args']
CopyDesc = STRUCTS['lime_copy_desc']
GatherDesc = STRUCTS['lime_gather_desc']
RankMetricsArgs = STRUCTS['lime_rank_metrics_args']
SlateMetricsArgs = STRUCTS['lime_slate_metrics_args']
ConvPoolArgs = STRUCTS['lime_conv_pool_args']

ABI_VERSION = CONSTANTS['LIME_ABI_VERSION']
MAX_COPIES = CONSTANTS['LIME_MAX_COPIES']
MAX_GATHERS = CONSTANTS['LIME_MAX_GATHERS']
NEG_MAX_K = CONSTANTS['LIME_NEG_MAX_K']
LIME_ACT = {None: CONSTANTS['LIME_ACT_NONE'], 'none': CONSTANTS['LIME_ACT_NONE'], 'relu': CONSTANTS['LIME_ACT_RELU'],
            'tanh': CONSTANTS['LIME_ACT_TANH'], 'sigmoid': CONSTANTS['LIME_ACT_SIGMOID'], 'relu_grad': CONSTANTS['LIME_ACT_RELU_GRAD']}
LINEAR_FAMILY = {CONSTANTS['LIME_LINEAR_NONE']: None, CONSTANTS['LIME_LINEAR_SP']: 'sp', CONSTANTS['LIME_LINEAR_PP']: 'pp',
                 CONSTANTS['LIME_LINEAR_MID']: 'mid', CONSTANTS['LIME_LINEAR_GENERAL']: 'general'}
ATTN_FORM = {f: CONSTANTS['LIME_ATTN_FORM_' + f.upper()] for f in ('plain', 'count', 'lse', 'rows', 'vocab', 'dropout')}
ATTN_FAMILY = {CONSTANTS['LIME_ATTN_' + f.upper()]: f for f in ('sp', 'sp_long', 'sp_vocab', 'mfma', 'wide', 'dropout', 'dropout_long')}
ATTN_FAMILY[CONSTANTS['LIME_ATTN_NONE']] = None
ATTN_STATS = {CONSTANTS['LIME_ATTN_STATS_NONE']: None, CONSTANTS['LIME_ATTN_STATS_FP32']: 'fp32', CONSTANTS['LIME_ATTN_STATS_SPLIT']: 'split'}
BWD_ATTN_ENTRY = {e: CONSTANTS['LIME_BWD_ATTN_ENTRY_' + e.upper()] for e in ('plain', 'lse')}
BWD_ATTN_FAMILY = {CONSTANTS['LIME_BWD_ATTN_' + f.upper()]: f for f in ('one_pass', 'sp', 'long', 'long_sp', 'wide')}
BWD_ATTN_FAMILY[CONSTANTS['LIME_BWD_ATTN_NONE']] = None
BWD_ATTN_PASS = {CONSTANTS['LIME_BWD_ATTN_PASS_NONE']: None, CONSTANTS['LIME_BWD_ATTN_PASS_STATS_FP32']: 'fp32',
                 CONSTANTS['LIME_BWD_ATTN_PASS_STATS_SPLIT']: 'split', CONSTANTS['LIME_BWD_ATTN_PASS_DELTA']: 'delta'}
LINEAR_PASS_RELU_BWD = CONSTANTS['LIME_LINEAR_PASS_RELU_BWD']
LINEAR_PASS_DROPOUT = CONSTANTS['LIME_LINEAR_PASS_DROPOUT']

_lib = None


def load():
    """Load liblime_hip.so once; raises if it is missing (build it with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LimeHipError('%s is missing: the HIP extension has not been built (run `python -c "import '
                           '__graft_entry__ as g; g.build()"` at the repo root); there is no CPU fallback' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    got = lib.lime_abi_version()
    if got != ABI_VERSION:
        raise LimeHipError('liblime_hip.so has ABI version %d, this binding expects %d' % (got, ABI_VERSION))
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().lime_last_error_string()
        raise LimeHipError('%s failed with status %d: %s' % (what, status, msg.decode() if msg else ''))
