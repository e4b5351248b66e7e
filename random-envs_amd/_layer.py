"""What the device-side layers above ``step()`` -- RolloutBuffer, ReplayBuffer, EpisodeLog -- share: the unwrapping of the env
they sit on, the pointer and stream plumbing of their ``rex_*`` calls and the checks of what callers hand them."""
import ctypes

from . import _native


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Layer:
    """Base of a layer over a :class:`VecRandomEnv` or a :class:`NormalizedVecRandomEnv`."""

    def __init__(self, env):
        import torch
        self._torch = torch
        self.env = env
        self._base = getattr(env, "env", env)      # the wrapped env of a NormalizedVecRandomEnv
        self._L, self._h = self._base._L, self._base._h
        self.batch, self.device = self._base.batch, self._base.device
        self.obs_dim, self.act_dim = int(self._base.dims.obs_dim), int(self._base.dims.act_dim)

    _p = staticmethod(_p)

    def _stream(self):
        return self._base._stream()

    def _check(self, t, shape, dtypes, name):
        if t.device != self.device or tuple(t.shape) != shape or t.dtype not in dtypes or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s tensor of %s on %s" % (type(self).__name__, name, list(shape), dtypes[0], self.device))

    def _check_index(self, index):
        t = self._torch
        if index.device != self.device or index.dtype != t.int64 or index.dim() != 1 or not index.is_contiguous():
            raise ValueError("%s.gather: index must be a contiguous 1-d int64 tensor on %s" % (type(self).__name__, self.device))

    def _read_counter(self, fn, clear):
        out = ctypes.c_int64()
        _native.check(fn(self._h, ctypes.byref(out), int(bool(clear))))
        return int(out.value)
