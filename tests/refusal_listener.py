"""A Context, or its library, that writes down what the library says when it refuses: the refusal tests of the GPU modules check codes and here and there a word
of the message; run on a Listening context they yield every text, whole and in order (tests/test_gpu_ssr_cacao_front_ends.py). It is the idea of _Listening in
tests/test_gpu_raster_front_ends.py, which notes the answers that a test asks for; this one also notes every refusal that the test does not ask about."""
import contextlib


class Listening:
    """`inner` (a Context, or its library). `asked` receives every answer of vqhip_last_error the caller asks for; `refused`, when given, receives
    (entry point, status, vqhip_last_error) after every library call that takes the context and returns a non-zero status, asked for or not"""
    def __init__(self, inner, asked, refused=None, handle=None):
        self._inner, self._asked, self._refused = inner, asked, refused
        if hasattr(inner, "lib"):
            self.lib = Listening(inner.lib, asked, refused, inner._h)
        self._handle = handle

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if name == "vqhip_last_error":
            def last_error(handle):
                text = attr(handle)
                self._asked.append((text or b"").decode())
                return text
            return last_error
        if self._refused is None or self._handle is None or not name.startswith("vqhip_"):
            return attr

        def call(*args):
            rc = attr(*args)
            if args and getattr(args[0], "value", args[0]) == self._handle.value and isinstance(rc, int) and rc != 0:
                self._refused.append((name, rc, (self._inner.vqhip_last_error(self._handle) or b"").decode()))
            return rc
        return call


@contextlib.contextmanager
def fresh_allocations():
    """Tensors made inside come from a memory pool of their own, so where they lie relative to each other depends on the code inside alone, not on what the
    process allocated and freed before. Which of two overlaps a refusal names depends on that"""
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
