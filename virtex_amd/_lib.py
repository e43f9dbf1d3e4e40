"""ctypes binding of libvirtex_amd.so (the C ABI declared in include/virtex_amd.h).

`import torch` happens first so that the HIP runtime already mapped by torch (its bundled
libamdhip64.so.7) is the one our library resolves against.

There is NO fallback: if the shared library is missing or a call fails, a RuntimeError is
raised.  The CPU fiber-emulator build of the same sources (tests/hipemu) can be selected
only explicitly, by tests, through `use_library()`.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (must precede loading the HIP library)

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "lib", "libvirtex_amd.so")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "virtex_amd.h")

_lib = None
_backend = None


class VtxError(RuntimeError):
    pass


# the header's closed set of types (every pointer but a `const char*` parameter is an address: c_void_p takes None, integers,
# bytes, arrays, byref(...) and string buffers)
_RETURNS = {"int": ctypes.c_int, "long": ctypes.c_long, "const char*": ctypes.c_char_p}
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
_POINTEES = {"void", "float", "int", "long", "long long", "double", "short", "unsigned short", "uint8_t", "unsigned char", "char",
             "VtxBnBwdFusion", "VtxAugParams", "VtxPrepDesc"}
_DECL = re.compile(r"(int|long|const char\s*\*)\s*\b(vtx_\w+)\s*\((.*)\)", re.S)
_PARAM = re.compile(r"(.*[\s*])(\w+)", re.S)


def _parse_header(text: str) -> dict:
    """{entry point: (restype, argtypes)} of every `vtx_*(...)` declaration of the header text.  A declaration or a type outside
    the forms above raises VtxError naming it: the binding never guesses."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    sigs = {}
    for stmt in text.split(";"):
        if not re.search(r"\bvtx_\w+\s*\(", stmt):
            continue
        decl = " ".join(stmt.split())
        m = _DECL.fullmatch(decl)
        if m is None:
            raise VtxError(f"include/virtex_amd.h: cannot bind declaration `{decl}`")
        argtypes = []
        for param in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            pm = _PARAM.fullmatch(param.strip())
            ctype = pm.group(1).replace(" *", "*").strip() if pm else ""
            if ctype == "const char*":
                argtypes.append(ctypes.c_char_p)
            elif ctype.endswith("*") and ctype[:-1].removeprefix("const ") in _POINTEES:
                argtypes.append(ctypes.c_void_p)
            elif ctype in _SCALARS:
                argtypes.append(_SCALARS[ctype])
            else:
                raise VtxError(f"include/virtex_amd.h: cannot bind parameter `{param.strip()}` of declaration `{decl}`")
        sigs[m.group(2)] = (_RETURNS[m.group(1).replace(" *", "*")], tuple(argtypes))
    return sigs


def use_library(path: str):
    """Load a specific build (tests use this to select the hipemu build) and declare every entry point's signature on it from
    include/virtex_amd.h: call sites pass plain Python values, and a call that disagrees with the header raises before it runs."""
    global _lib, _backend
    if not os.path.exists(path):
        raise VtxError(
            f"virtex_amd native library not found at {path}; run `python -m virtex_amd.build` "
            "(the HIP extension is mandatory: there is no CPU/PyTorch fallback)")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    with open(_HEADER) as fh:
        sigs = _parse_header(fh.read())
    for name, (restype, argtypes) in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    _backend = lib.vtx_backend().decode()
    return lib


def lib():
    if _lib is None:
        use_library(os.environ.get("VIRTEX_AMD_LIB", DEFAULT_LIB))
    return _lib


def backend() -> str:
    lib()
    return _backend


def is_emulator() -> bool:
    return backend() == "hipemu"


_recorder = None     # virtex_amd.replay.Recorder while a step is being recorded (launch replay), else None


def set_recorder(rec):
    global _recorder
    _recorder = rec


def call(name: str, *args):
    """Invoke a C-ABI entry point; raise VtxError(vtx_last_error()) on non-zero status."""
    fn = getattr(lib(), name)
    if len(args) != len(fn.argtypes):    # (ctypes itself lets surplus arguments of a cdecl function through)
        raise VtxError(f"{name} takes {len(fn.argtypes)} arguments (include/virtex_amd.h), {len(args)} given")
    try:
        rc = fn(*args)
    except ctypes.ArgumentError as e:    # "argument <index>: <what was wrong>", raised before the call is made
        raise VtxError(f"{name}: {e}") from None
    if rc != 0:
        raise VtxError(f"{name} failed ({rc}): {lib().vtx_last_error().decode()}")
    if _recorder is not None:            # the same call, re-issued by virtex_amd.replay (plain values: the argtypes convert them again)
        def again(f=fn, a=args, n=name):
            if f(*a) != 0:               # a launch that fails during a replay raises exactly as the eager call does
                raise VtxError(f"{n} failed during launch replay: {lib().vtx_last_error().decode()}")
        _recorder.add("kernel", again, args, label=name)


# torch.cuda.current_stream() builds a Stream object through three Python layers (4.4 us per call, 2.5 ms of the 12 ms the
# host spends per step: tools/host_profile.py); the raw handle is one C call
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream_handle(device) -> int:
    """hipStream_t (as an integer) of torch's current stream on `device`."""
    if _raw_stream is not None:
        idx = device.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(device).cuda_stream


def _device_stream(device) -> int:
    """hipStream_t (as an integer) that work for `device` is enqueued on: torch's current stream, 0 for the emulator's CPU tensors."""
    return current_stream_handle(device) if device.type == "cuda" else 0


def stream_ptr(t: torch.Tensor) -> int:
    """hipStream_t the work for tensor `t` must be enqueued on."""
    if t.is_cuda:
        return current_stream_handle(t.device)
    if not is_emulator():
        raise VtxError("CPU tensor passed to the HIP build of virtex_amd (no CPU fallback exists)")
    return 0


def ptr(t) -> int:
    """Device address of a tensor (None -> NULL)."""
    if t is None:
        return 0
    if _recorder is not None:
        _recorder.keep.append(t)         # the recorded launch holds this address: the tensor must outlive the recording
    return t.data_ptr()


VTX_F32, VTX_BF16 = 0, 1


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return VTX_F32
    if dt == torch.bfloat16:
        return VTX_BF16
    raise VtxError(f"unsupported dtype {dt}")
