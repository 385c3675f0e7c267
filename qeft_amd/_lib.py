"""ctypes binding of the C ABI in include/qeft_hip.h (qeft_amd/lib/libqeft_hip.so).

There is no CPU fallback: if the library is missing, or an entry point fails, the call raises.
"""
import ctypes
import os
import re

# torch must be in the process BEFORE the library is loaded: torch ships its own libamdhip64 and the library links
# the system one under the same soname.  Whichever loads first serves both; if it is the system copy, torch's
# streams / allocations and this library's kernels end up in two HIP runtimes and every launch fails
# (hipErrorNoDevice).  Loading torch first makes its runtime the only one.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# QEFT_HIP_LIB: load another build of the same ABI (A/B timing of two builds on one GPU box); never a fallback
LIB_PATH = os.environ.get("QEFT_HIP_LIB") or os.path.join(_HERE, "lib", "libqeft_hip.so")

HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "qeft_hip.h"))


class QeftHipError(RuntimeError):
    pass


_ARG = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong, "qeft_stream_t": ctypes.c_void_p}
_RET = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}


def parse_header(text):
    """[(name, restype, argtypes)] of every `ret qeft_name(params);` in the header text, in order of declaration.
    A pointer of any kind is c_void_p; a type that neither table knows raises -- a guess here would truncate a device address."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)                    # some sit inside parameter lists
    text = re.sub(r"//[^\n]*|^[ \t]*#[^\n]*", " ", text, flags=re.M)
    protos = []
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(qeft_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RET:
            raise QeftHipError(f"{name}: return type '{ret}' has no ctypes mapping")
        argtypes = []
        for param in (params.split(",") if params.strip() != "void" else []):
            words = param.split()                                        # the last one is the parameter's name
            ctype = ctypes.c_void_p if "*" in param else _ARG.get(" ".join(words[:-1]))
            if ctype is None:
                raise QeftHipError(f"{name}: parameter '{' '.join(words)}' has no ctypes mapping")
            argtypes.append(ctype)
        protos.append((name, _RET[ret], argtypes))
    return protos


def _read_header():
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise QeftHipError(f"{HEADER} not readable ({e}): the ctypes binding is derived from it") from None


# name -> argtypes / restype, as include/qeft_hip.h declares them
_PROTOS = parse_header(_read_header())
SIGNATURES = {name: argtypes for name, _, argtypes in _PROTOS}
RESTYPES = {name: restype for name, restype, _ in _PROTOS}

_lib = None


def lib():
    """Load (once) and return the CDLL.  Raises if the HIP library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QeftHipError(
                f"{LIB_PATH} not found: build it with `python -m qeft_amd.build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the quantized linear.")
        l = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(l, name, None)
            if fn is None:
                # only an explicitly selected A/B build (QEFT_HIP_LIB) may be older than the header; the in-tree library must
                # export every entry
                if os.environ.get("QEFT_HIP_LIB"):
                    continue
                raise QeftHipError(f"{LIB_PATH} does not export {name}: rebuild it (python -m qeft_amd.build)")
            fn.argtypes = argtypes
            fn.restype = RESTYPES[name]
        _lib = l
    return _lib


def last_variant():
    """Kernel variant the calling thread's last compute entry dispatched to (qeft_last_variant)."""
    return lib().qeft_last_variant().decode()


def check(code):
    if code != 0:
        l = lib()
        msg = l.qeft_error_string(code).decode()
        if code == 5:
            msg += f" (hipError_t={l.qeft_last_hip_error()})"
        raise QeftHipError(msg)
