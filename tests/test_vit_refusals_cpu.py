"""CPU check that the ViT launch layer refuses what it refused before (csrc/vit.hip: the plain, training and dropout forms of one operation share a host body).

For each of the sixteen entries below (the token GEMM and the attention, forward and backward, in their plain, training and dropout forms, and dropout on
rows) an otherwise valid argument list is built: M = 1, K = N = 256; B = 1, one token, one query row; 16-byte-aligned host buffers; the workspace size the
entry's own *_workspace_bytes names.  That list must get past every check, which without a device ends as CVAE_E_LAUNCH.  Then one argument at a time is
replaced according to its ctype in _lib.SIGNATURES:
    pointer: null, base + 4        int64: 0, -1, 3, 2^40        int: -1, 7        float (a rate): -0.1, 1.0, NaN        size_t: 0
and, as one pair, the row or batch count is set to 0 together with a null first pointer (the header's rule: the shape is judged first).
The expected codes are data: tests/golden/vit_refusals.json, recorded from the library of the commit before the bodies were merged by running this file
as a script with CVAE_HIP_LIB naming that library.  pytest only compares; it never writes the file.
The whole file is skipped where a device exists, as test_launch_layer_cpu.py is: a missed check can then only end as CVAE_E_LAUNCH, never as a launch on host
pointers."""
import ctypes as C
import json
import math
import os
import sys

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("host pointers stand in for device memory: only where no launch can succeed", allow_module_level=True)

if __name__ == "__main__":                          # run as a script, the package is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from causal_vae_amd import _lib  # noqa: E402

lib = _lib.lib
F, BF = _lib.F32, _lib.BF16
E_LAUNCH = -5
CODES = {"CVAE_E_BADSHAPE": -1, "CVAE_E_DTYPE": -2, "CVAE_E_UNSUPPORTED": -3, "CVAE_E_WORKSPACE": -4, "CVAE_E_NULLPTR": -6}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_refusals.json")

_buf = (C.c_char * (1 << 16))()                     # never read or written through: no launch succeeds here
P = (C.addressof(_buf) + 15) & ~15
KEY = 0x1234567890ABCDEF
WS = lib.cvae_mhsa_bwd_workspace_bytes(1, 1)
QKV = (256,) * 3 + (0,) * 3                         # row strides, batch strides

# (entry, the variant's name, the otherwise valid arguments, the position of the row or batch count)
BASES = [
    ("cvae_token_gemm", "plain-bf16", (P, 256, P, P, None, 0, P, 256, 1, 256, 256, 0, BF, None), 8),
    ("cvae_token_gemm", "residual", (P, 256, P, P, P, 256, P, 256, 1, 256, 256, 2, F, None), 8),
    ("cvae_token_gemm_gelu_train", "f32", (P, 256, P, P, P, 256, P, 256, 1, 256, 256, F, None), 8),
    ("cvae_token_gemm_dropout", "gelu", (P, 256, P, P, None, 0, P, 256, P, 256, 1, 256, 256, 1, 0.1, KEY, 0, 1, None), 10),
    ("cvae_token_gemm_dropout", "residual", (P, 256, P, P, P, 256, None, 0, P, 256, 1, 256, 256, 2, 0.1, KEY, 0, 1, None), 10),
    ("cvae_token_gemm_dropout_devkey", "gelu", (P, 256, P, P, None, 0, P, 256, P, 256, 1, 256, 256, 1, 0.1, P, 0, 1, None), 10),
    ("cvae_token_gemm_dropout_devkey", "residual", (P, 256, P, P, P, 256, None, 0, P, 256, 1, 256, 256, 2, 0.1, P, 0, 1, None), 10),
    ("cvae_mhsa_fwd", "f32", (P,) * 4 + QKV + (1, 1, 1, F, None), 10),
    ("cvae_mhsa_fwd_train", "bf16", (P,) * 5 + QKV + (1, 1, 1, BF, None), 11),
    ("cvae_mhsa_fwd_train_dropout", "f32", (P,) * 5 + QKV + (1, 1, 1, 0.1, KEY, None), 11),
    ("cvae_mhsa_fwd_train_dropout_devkey", "f32", (P,) * 5 + QKV + (1, 1, 1, 0.1, P, None), 11),
    ("cvae_mhsa_bwd", "f32", (P,) * 9 + QKV * 2 + (1, 1, 1, F, P, WS, None), 21),
    ("cvae_mhsa_bwd", "bf16", (P,) * 9 + QKV * 2 + (1, 1, 1, BF, P, WS, None), 21),
    ("cvae_mhsa_bwd_dropout", "f32", (P,) * 9 + QKV * 2 + (1, 1, 1, 0.1, KEY, P, WS, None), 21),
    ("cvae_mhsa_bwd_dropout_devkey", "f32", (P,) * 9 + QKV * 2 + (1, 1, 1, 0.1, P, P, WS, None), 21),
    ("cvae_token_gemm_bwd_data", "f32-gated-residual", (P, 256, F, P, P, 256, P, 256, P, 256, F, 1, 256, 256, F, None), 11),
    ("cvae_token_gemm_bwd_data", "bf16-plain", (P, 256, BF, P, None, 0, None, 0, P, 256, F, 1, 256, 256, BF, None), 11),
    ("cvae_token_gemm_bwd_data_dropout", "gated", (P, 256, P, P, 256, P, 256, 1, 256, 256, 0.1, KEY, 0, 1, None), 7),
    ("cvae_token_gemm_bwd_data_dropout_devkey", "gated", (P, 256, P, P, 256, P, 256, 1, 256, 256, 0.1, P, 0, 1, None), 7),
    ("cvae_dropout_rows", "f32", (P, 256, P, 256, 1, 256, 0.1, KEY, 0, 1, None), 4),
    ("cvae_dropout_rows_devkey", "f32", (P, 256, P, 256, 1, 256, 0.1, P, 0, 1, None), 4),
]
ENTRIES = sorted({b[0] for b in BASES})
IDS = [f"{name}-{variant}" for name, variant, _a, _c in BASES]

REPLACEMENTS = {
    C.c_void_p: lambda base: (("null", None), ("base+4", (base or 0) + 4)),
    C.c_int64: lambda base: (("0", 0), ("-1", -1), ("3", 3), ("2^40", 1 << 40)),
    C.c_int: lambda base: (("-1", -1), ("7", 7)),
    C.c_float: lambda base: (("-0.1", -0.1), ("1.0", 1.0), ("nan", math.nan)),
    C.c_size_t: lambda base: (("0", 0),),
}


def cases(name, args, count_at):
    """(label, argument list) of every replacement of one base list (the stream is a pointer like the others: no entry judges it)"""
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(args) and sig[count_at] is C.c_int64 and sig[0] is C.c_void_p
    for i, ct in enumerate(sig):
        for label, value in REPLACEMENTS.get(ct, lambda base: ())(args[i]):
            yield f"arg{i}={label}", args[:i] + (value,) + args[i + 1:]
    zero = list(args)
    zero[0], zero[count_at] = None, 0
    yield f"arg{count_at}=0,arg0=null", tuple(zero)


def answers(name, args, count_at):
    fn = getattr(lib, name)
    return {label: fn(*a) for label, a in cases(name, args, count_at)}


def record():
    return {f"{name}/{variant}": answers(name, args, count_at) for name, variant, args, count_at in BASES}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_names_every_entry_and_every_code(golden):
    assert len(ENTRIES) == 16 and all(n in _lib.SIGNATURES for n in ENTRIES)
    assert sorted(golden) == sorted(f"{name}/{variant}" for name, variant, _a, _c in BASES)
    seen = {code for table in golden.values() for code in table.values()}
    assert set(CODES.values()) <= seen, {k for k, v in CODES.items() if v not in seen}


@pytest.mark.parametrize("name,variant,args,count_at", BASES, ids=IDS)
def test_every_refusal_is_the_recorded_one(golden, name, variant, args, count_at):
    assert getattr(lib, name)(*args) == E_LAUNCH, f"{name}: the arguments are not otherwise valid"
    want, got = golden[f"{name}/{variant}"], answers(name, args, count_at)
    assert sorted(got) == sorted(want), "the recorded table holds other cases than this file builds"
    wrong = {label: (got[label], want[label]) for label in got if got[label] != want[label]}
    assert not wrong, f"{name}/{variant}: (answer, recorded answer) differ for {wrong}"
    assert any(code != E_LAUNCH for code in got.values())


if __name__ == "__main__":
    table = record()
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{GOLDEN}: {sum(len(t) for t in table.values())} answers of {_lib.LIB_PATH}")
