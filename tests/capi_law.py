"""The C ABI as the compiler reads it, and the rule a ctypes call has to keep against it.

include/hyperpocket_hip.h is the one statement of the library's door.  The Python side sets no argtypes: every call site
hands ctypes objects of its own choosing, so a `long long`, a `double` or a pointer that gets a 4-byte object is read wrong
only when the neighbouring bytes are not zero (a stack slot keeps its upper half, an xmm register its upper lanes).  This
module states, once:

  prototypes()             per hp_* name the return class and the parameter classes (ptr, i32, i64, f32, f64), deduced by a
                           host C++17 program from decltype(&hp_x): the classes are the compiler's, the names the regex of
                           tests/test_capi_symbols.py
  struct_layouts(lines)    sizeof and (name, offsetof, size) of every field of the header's Hp* structs as the files named by
                           the given #include lines state them
  compatible(decl, obj)    whether ctypes marshals obj as a parameter of class decl
  returns_ok(decl, restype)whether a function object with that restype reads a return of class decl whole
  checked_library()        the loaded library behind a proxy that holds every call to the above and records it
"""
import contextlib
import ctypes
import functools
import os
import re
import shutil
import subprocess
import tempfile

from conftest import PKG_DIR, ROOT

HEADER = os.path.join(ROOT, "include", "hyperpocket_hip.h")
CSRC = os.path.join(PKG_DIR, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLASSES = ("ptr", "i32", "i64", "f32", "f64")
STRUCTS = ("HpGemmDesc", "HpEncoderWeights", "HpEncoderGrads", "HpHyperWeights", "HpHyperGrads", "HpEncoderIO",
           "HpEncoderBwdIO", "HpEncoderPlan", "HpHeadsPlan", "HpRenderPlan")
JOBS = 16


def declared():
    from test_capi_symbols import _declared
    return _declared()


def _run_program(source, suffix=".cpp", include_dirs=()):
    """Compile a host-only program and return what it prints.  The host compiler where the text is plain C++; hipcc's host
    pass where it includes a .hip file."""
    tmp = tempfile.mkdtemp(prefix="capi_law_")
    try:
        src, exe = os.path.join(tmp, "probe" + suffix), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(source)
        incs = [f"-I{d}" for d in include_dirs]
        cxx = shutil.which("c++") or shutil.which("g++")
        if suffix == ".cpp" and cxx:
            cmd = [cxx, "-std=c++17", "-O0", "-w"] + incs + [src, "-o", exe]
        else:
            cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-x", "hip", "-std=c++17", "-O0", "-w"] + incs + [src, "-o", exe]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed:\n{done.stderr[-4000:]}")
        return subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


_CLASS_OF = """
#include <cstdio>
#include <cstddef>
#include <type_traits>
template <class T> const char* class_of() {
    if (std::is_void<T>::value) return "void";
    if (std::is_pointer<T>::value) return "ptr";
    if (std::is_floating_point<T>::value) return sizeof(T) == 8 ? "f64" : sizeof(T) == 4 ? "f32" : "other";
    if (std::is_integral<T>::value || std::is_enum<T>::value) return sizeof(T) == 8 ? "i64" : sizeof(T) == 4 ? "i32" : "other";
    return "other";
}
template <> const char* class_of<void>() { return "void"; }
template <class F> struct Show;
template <class R, class... A> struct Show<R (*)(A...)> {
    static void line(const char* name) {
        const char* args[] = {class_of<A>()..., nullptr};
        std::printf("%s %s", name, class_of<R>());
        for (int i = 0; args[i]; ++i) std::printf(" %s", args[i]);
        std::printf("\\n");
    }
};
"""


@functools.lru_cache(maxsize=None)
def prototypes():
    """{name: (return class, (parameter class, ...))} for every declared hp_* entry point."""
    names = declared()
    body = "".join(f'    Show<decltype(&{n})>::line("{n}");\n' for n in names)
    out = _run_program(f'#include "hyperpocket_hip.h"\n{_CLASS_OF}\nint main() {{\n{body}    return 0;\n}}\n',
                       include_dirs=[os.path.dirname(HEADER)])
    table = {}
    for line in out.splitlines():
        name, ret, *params = line.split()
        table[name] = (ret, tuple(params))
    assert sorted(table) == names
    for name, (ret, params) in table.items():
        assert ret in CLASSES + ("void",) and all(p in CLASSES for p in params), (name, ret, params)
    return table


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def struct_fields(text, struct):
    """The field names of `struct` in C text, in order, or None if the text does not define it.  Only the names come from
    here: the program of struct_layouts unpacks the struct into exactly these names (a structured binding, which the compiler
    refuses at any other count) and takes every offset and size from the compiler."""
    m = re.search(r"\bstruct\s+%s\s*\{(.*?)\}" % struct, _strip_comments(text), flags=re.S)
    if m is None:
        return None
    names = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for piece in decl.split(","):
            piece = re.sub(r"\[[^\]]*\]", "", piece).strip()
            names.append(re.search(r"([A-Za-z_]\w*)\s*$", piece).group(1))
    return names


def _included_text(include_lines):
    text = ""
    for line in include_lines:
        m = re.match(r'\s*#\s*include\s+"([^"]+)"', line)
        if m:
            for d in (os.path.dirname(HEADER), CSRC):
                if os.path.exists(os.path.join(d, m.group(1))):
                    text += open(os.path.join(d, m.group(1))).read() + "\n"
                    break
    return text


@functools.lru_cache(maxsize=None)
def struct_layouts(include_lines):
    """{struct: {"size": sizeof, "fields": [(name, offsetof, sizeof), ...]}} for each of STRUCTS that the files named by
    `include_lines` (a tuple of #include lines, resolved against include/ and csrc/) define."""
    text = _included_text(include_lines)
    found = {s: struct_fields(text, s) for s in STRUCTS}
    found = {s: f for s, f in found.items() if f is not None}
    # a .hip file does not link without its device image: of one, the program gets the Hp* struct statements alone, verbatim
    lines = []
    for line in include_lines:
        if ".hip" in line:
            own = _strip_comments(_included_text((line,)))
            lines += [m.group(0) for s in STRUCTS for m in re.finditer(r"\bstruct\s+%s\s*\{.*?\}\s*\w*\s*;" % s, own, flags=re.S)]
        else:
            lines.append(line)
    prog = "\n".join(lines) + "\n" + _CLASS_OF
    for s, fields in found.items():
        prog += f"void count_{s}({s}& v) {{ auto& [{', '.join('f%d' % i for i in range(len(fields)))}] = v; }}\n"
    prog += "int main() {\n"
    for s, fields in found.items():
        prog += f'    std::printf("{s} %zu\\n", sizeof({s}));\n'
        for f in fields:
            prog += f'    std::printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));\n'
    prog += "    return 0;\n}\n"
    hip = any(os.path.basename(HEADER) not in line for line in include_lines)      # csrc text wants the HIP runtime's types
    out = _run_program(prog, suffix=".hip" if hip else ".cpp", include_dirs=[os.path.dirname(HEADER), CSRC])
    layouts = {}
    for line in out.splitlines():
        key, *nums = line.split()
        if "." in key:
            s, f = key.split(".")
            layouts[s]["fields"].append((f, int(nums[0]), int(nums[1])))
        else:
            layouts[key] = {"size": int(nums[0]), "fields": []}
    return layouts


def ctypes_layout(cls):
    """A ctypes.Structure in the form of struct_layouts."""
    return {"size": ctypes.sizeof(cls),
            "fields": [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, *_ in cls._fields_]}


# ------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------
_INT_CODES = "bBhHiIlLqQ"
_CARG = type(ctypes.byref(ctypes.c_int()))


def _int_bytes(obj_or_type):
    """Size of a ctypes integer object or type, 0 for anything else (c_bool, c_char and c_void_p are no integers here)."""
    t = obj_or_type if isinstance(obj_or_type, type) else type(obj_or_type)
    if not (isinstance(t, type) and issubclass(t, ctypes._SimpleCData)) or getattr(t, "_type_", "") not in _INT_CODES:
        return 0
    return ctypes.sizeof(t)


def seen(actual):
    """A short name of what ctypes is handed, for the record and the messages."""
    if actual is None:
        return "None"
    if type(actual) in (int, bool):
        return f"{type(actual).__name__}({actual})"
    return type(actual).__name__


def compatible(declared_class, actual):
    """Does ctypes, with no argtypes set, marshal `actual` as a parameter of class `declared_class`?  `actual` is the object
    the foreign function is called with (after _lib.call's conversion).
      i32  c_int, c_uint, c_bool, or a bare Python int within int32 (ctypes marshals that as c_int)
      i64  an 8-byte ctypes integer only: a bare int or a c_int fills four bytes of the eight
      f32  c_float only
      f64  c_double only
      ptr  c_void_p, None, a ctypes pointer, array or byref object, or an 8-byte ctypes integer; never a bare int (0
           included) and never c_int"""
    t = type(actual)
    if declared_class == "i32":
        if t in (ctypes.c_int, ctypes.c_uint, ctypes.c_bool):
            return True
        return t in (int, bool) and -2 ** 31 <= int(actual) < 2 ** 31
    if declared_class == "i64":
        return _int_bytes(actual) == 8
    if declared_class == "f32":
        return t is ctypes.c_float
    if declared_class == "f64":
        return t is ctypes.c_double
    if declared_class == "ptr":
        if actual is None or t in (ctypes.c_void_p, ctypes.c_char_p, ctypes.c_wchar_p, _CARG):
            return True
        if isinstance(actual, (ctypes._Pointer, ctypes.Array, ctypes._CFuncPtr)):
            return True
        return _int_bytes(actual) == 8
    raise ValueError(declared_class)


def returns_ok(declared_class, restype):
    """Does a function object whose restype is `restype` (ctypes' default is c_int) read a return of `declared_class` whole?"""
    if declared_class == "void":
        return True
    if declared_class == "i32":
        return restype in (ctypes.c_int, ctypes.c_uint)
    if declared_class == "i64":
        return _int_bytes(restype) == 8 if isinstance(restype, type) else False
    if declared_class == "f32":
        return restype is ctypes.c_float
    if declared_class == "f64":
        return restype is ctypes.c_double
    if declared_class == "ptr":
        if restype in (ctypes.c_void_p, ctypes.c_char_p):
            return True
        return isinstance(restype, type) and (issubclass(restype, ctypes._Pointer) or _int_bytes(restype) == 8)
    raise ValueError(declared_class)


def check_call(name, args, restype, table=None):
    """The violations of one call as strings (empty: the call keeps the rule)."""
    table = table or prototypes()
    if name not in table:
        return [f"{name}: not declared in the header"]
    ret, params = table[name]
    bad = []
    if len(args) != len(params):
        bad.append(f"{name}: {len(args)} arguments for {len(params)} parameters")
    for i, (p, a) in enumerate(zip(params, args)):
        if not compatible(p, a):
            bad.append(f"{name}: argument {i} is declared {p} and gets {seen(a)}")
    if not returns_ok(ret, restype):
        bad.append(f"{name}: returns {ret} and is read through restype {getattr(restype, '__name__', restype)}")
    return bad


# ------------------------------------------------------------------------------------------------------------------------
# the checking library
# ------------------------------------------------------------------------------------------------------------------------
class _CheckedFunction:
    """Stands where a ctypes function object stands: a call is checked, recorded and forwarded with the very objects it was
    given; restype, argtypes and errcheck are those of the real function object."""

    def __init__(self, name, real, log):
        object.__setattr__(self, "_name", name)
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_log", log)

    def __call__(self, *args):
        self._log.calls.append((self._name, tuple(seen(a) for a in args)))
        self._log.violations.extend(check_call(self._name, args, self._real.restype))
        return self._real(*args)

    def __getattr__(self, attr):
        return getattr(self._real, attr)

    def __setattr__(self, attr, value):
        setattr(self._real, attr, value)


class _CheckedLibrary:
    def __init__(self, real, log):
        self._real, self._log, self._fns = real, log, {}

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if not name.startswith("hp_"):
            return real
        fn = self._fns.get(name)
        if fn is None:
            fn = self._fns[name] = _CheckedFunction(name, real, self._log)
        return fn

    def __getitem__(self, name):
        return getattr(self, name)


class CallLog:
    def __init__(self):
        self.calls, self.violations = [], []

    def names(self):
        return {name for name, _ in self.calls}


@contextlib.contextmanager
def checked_library(log=None):
    """Inside the block hyperpocket_amd's library is a fresh CDLL (fresh function objects: no restype survives from an
    earlier caller) behind the checking proxy; yields the CallLog.  A violation is collected, not raised, so that one run
    lists them all.  Objects that keep the library (the engine) have to be made inside the block."""
    from hyperpocket_amd import _lib
    log = log if log is not None else CallLog()
    saved_lib, saved_fn = _lib._LIB, dict(_lib._FN)
    _lib._LIB = None
    try:
        real = _lib.load_library()
        _lib._LIB = _CheckedLibrary(real, log)
        _lib._FN.clear()
        yield log
    finally:
        _lib._LIB = saved_lib
        _lib._FN.clear()
        _lib._FN.update(saved_fn)
