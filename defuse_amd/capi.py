"""What every ctypes binding of include/*.h shares: the status codes, the one place that sets argtypes / restype, the error
base, and the base of the classes that own a C handle.  Imports neither torch nor dsa."""
import ctypes

E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT, E_BUSY = -1, -2, -3, -4, -5      # DSA_E_* of include/defuse_dsa.h

_bound = {}      # (id(lib), id(table)) -> (lib, table): held, so that the ids stay theirs


def bind(lib, prototypes):
    """Sets argtypes and restype of every function of `prototypes`, {name: (restype, [argtypes...])}, on `lib` and returns
    `lib`; a second call for the same library and table does nothing.  A name the library lacks raises AttributeError."""
    key = (id(lib), id(prototypes))
    if key not in _bound:
        for name, (restype, argtypes) in prototypes.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        _bound[key] = (lib, prototypes)
    return lib


class ApiError(RuntimeError):
    """A negative return code of the C ABI; a subclass gives its prefix."""
    prefix = "api"

    def __init__(self, code, msg):
        super().__init__("%s error %d: %s" % (self.prefix, code, msg))
        self.code = code


def ptr(a):
    """The address of a numpy array's data, NULL for an empty one."""
    return a.ctypes.data if len(a) else None


def as_dict(struct):
    """A timing struct as a dict, without its padding."""
    return {name: getattr(struct, name) for name, *_ in struct._fields_ if name != "pad_"}


class Owned:
    """Base of a class that owns one C handle: a subclass names its destroy function in `_destroy`, calls
    Owned.__init__(self, lib) and then lets the library fill self.handle."""
    _destroy = None
    _lib = None
    handle = None      # (a half-constructed object has nothing to free)

    def __init__(self, lib):
        self._lib = lib
        self.handle = ctypes.c_void_p()

    def close(self):
        if self.handle:
            getattr(self._lib, self._destroy)(self.handle)
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: the library or ctypes may be gone already
            pass
