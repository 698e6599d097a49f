"""Poisoned, guard-banded allocations for ``HipBackend`` (tests only; nothing here launches a kernel or needs a GPU to be imported).

``HipBackend`` allocates every output and every scratch buffer through the module-level name ``torch`` of ``op/_backend.py`` and calls every
kernel entry through ``HipBackend._launch``.  ``guarded(backend_module, poison)`` swaps that name for a proxy whose ``empty`` / ``empty_like`` /
``zeros`` hand out views into buffers the test owns,

    | guard (canary words) | payload (poison, or zeros for ``zeros``) | guard (canary words) |

and wraps ``_launch`` so that the entry names called inside the context are recorded.  ``check()`` then says which guard words changed: a store
outside the granted bytes.  A kernel that reads an output or a workspace before writing it shows up as NaN (``'nan'`` poison) or as a result that
differs between the two poisons (``'big'``: 1e30, finite, so that a poison that is multiplied by zero or masked away is seen by comparison).

Layout rules (conditions, not measurements): the payload starts on a 512-byte boundary -- what the caching allocator hands out, so alignment-dependent
kernel paths run as in production; the trailing guard starts at the first 4-byte word after the payload's last byte, NOT rounded up, so a one-element
overrun lands in it; each guard is as large as the payload rounded up to 512 B and never below 64 KiB (more than any single tile-row overrun of the
shapes under test; one whole extra channel block, sample or K slice still lands in owned memory).

The READ side: ``hostile(t, fill, shift)`` places a copy of an INPUT in the same layout, with ``fill`` (a word of ``FILLS``: NaN, 1e30 or zero) in
both guards and in every byte between the logical elements of a non-dense view, optionally ``shift`` bytes off the 512-byte boundary; and
``guarded(..., canary=word)`` writes that word into the guards of every backend allocation, so that an intermediate reaches the next kernel with
the same neighbourhood.  A kernel whose result depends on a byte outside its input's logical elements then gives NaN, or results that differ
between the fills.  Nothing is placed against unmapped memory: an out-of-input read shows in values, never as a fault.
"""
import contextlib
import struct
import sys

import torch as _torch

CANARY = 0x5CA1AB1E                    # every 32-bit word of a guard
POISONS = {'nan': 0x7FC00000,          # quiet NaN
           'big': struct.unpack('<i', struct.pack('<f', 1e30))[0]}          # 1e30f: finite, and no sum of products of test-sized values comes near it
FILLS = dict(POISONS, zero=0)           # what hostile() puts around an input
ALIGN = 512
MIN_GUARD = 64 << 10


def _round_up(v, m):
    return (v + m - 1) // m * m


def _storage_elems(shape, strides):
    """Elements a view with these extents and strides spans (0 for an empty one)."""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, strides))


def _contiguous_strides(shape):
    out, acc = [], 1
    for s in reversed(shape):
        out.append(acc)
        acc *= max(s, 1)
    return tuple(reversed(out))


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


class Allocation:
    """One harness allocation: the backing buffer (kept alive), where its three regions are, and who asked for it."""
    __slots__ = ('backing', 'front', 'back', 'payload_words', 'shape', 'dtype', 'nbytes', 'function', 'line', 'kind')

    def describe(self):
        return '%s%s %s at %s:%d' % (self.kind, list(self.shape), str(self.dtype).replace('torch.', ''), self.function, self.line)


class Guard:
    """What ``guarded()`` yields: the allocator (``empty`` / ``empty_like`` / ``zeros``: also for buffers a TEST hands to a primitive), the list of
    allocations, the recorded entry names and ``check()``."""

    def __init__(self, poison, canary=CANARY):
        if poison not in POISONS:
            raise ValueError('poison must be one of %s, got %r' % (sorted(POISONS), poison))
        if not (isinstance(canary, int) and 0 <= canary < 1 << 31):
            raise ValueError('canary must be a non-negative int32 word, got %r' % (canary,))
        self.poison = poison
        self.canary = canary          # every 32-bit word of every guard; compared as int32 bits (a NaN word never equals itself as a float)
        self.allocations = []
        self.entries = []

    # -- allocation ------------------------------------------------------------------------------------------------------------------
    def _requester(self):
        """(function, line) of the frame that called the proxy: the first one outside this module."""
        f = sys._getframe(2)
        while f is not None and f.f_code.co_filename == __file__:
            f = f.f_back
        return (f.f_code.co_name, f.f_lineno) if f is not None else ('?', 0)

    def _allocate(self, kind, shape, strides, dtype, device, fill_word):
        dtype = _torch.float32 if dtype is None else dtype
        device = _torch.device('cpu' if device is None else device)
        itemsize = _torch.empty(0, dtype=dtype).element_size()
        nbytes = _storage_elems(shape, strides) * itemsize
        guard = max(MIN_GUARD, _round_up(nbytes, ALIGN))
        words = _round_up(nbytes, 4) // 4
        # ALIGN spare bytes: wherever the backing buffer starts (the host allocator aligns to 64 B only), a 512-byte boundary with a whole guard in front fits
        backing = _torch.empty((guard + ALIGN + 4 * words + guard) // 4, dtype=_torch.int32, device=device)
        start = (_round_up(backing.data_ptr() + guard, ALIGN) - backing.data_ptr()) // 4          # payload, in words from the backing buffer's first
        backing.fill_(self.canary)
        rec = Allocation()
        rec.backing, rec.shape, rec.dtype, rec.nbytes, rec.kind = backing, tuple(shape), dtype, nbytes, kind
        rec.front, rec.back, rec.payload_words = backing[start - guard // 4:start], backing[start + words:start + words + guard // 4], words
        rec.function, rec.line = self._requester()
        payload = backing[start:start + words]
        if fill_word == 0:
            payload.zero_()
        elif dtype == _torch.float32:
            payload.fill_(fill_word)
        else:
            payload.fill_(-1)              # 0xFF bytes
        self.allocations.append(rec)
        return _torch.as_strided(payload.view(_torch.uint8)[:nbytes].view(dtype), shape, strides)

    def empty(self, *size, dtype=None, device=None, **kw):
        self._no_extras(kw)
        shape = _shape_of(size)
        return self._allocate('empty', shape, _contiguous_strides(shape), dtype, device, POISONS[self.poison])

    def zeros(self, *size, dtype=None, device=None, **kw):
        self._no_extras(kw)
        shape = _shape_of(size)
        return self._allocate('zeros', shape, _contiguous_strides(shape), dtype, device, 0)

    def empty_like(self, t, dtype=None, device=None, **kw):
        self._no_extras(kw)
        like = _torch.empty_like(t, device='meta')        # the strides the real call gives (dense inputs keep theirs, anything else becomes contiguous)
        return self._allocate('empty_like', tuple(like.shape), tuple(like.stride()), t.dtype if dtype is None else dtype,
                              t.device if device is None else device, POISONS[self.poison])

    @staticmethod
    def _no_extras(kw):
        if kw:
            raise TypeError('guarded allocation: unsupported arguments %s (teach tests/guarded_alloc.py about them)' % sorted(kw))

    # -- verification ----------------------------------------------------------------------------------------------------------------
    def _compare(self, words):
        """Mask of the guard words that no longer hold the canary."""
        return words != self.canary

    def check(self):
        """Synchronise and compare every guard.  -> [violation]: dicts with the requesting ``function`` and ``line``, the ``shape``, the ``side``
        ('before' | 'after'), ``offset`` (bytes from the payload to the first corrupted word: -4 is the word just in front of the payload's first
        byte, 0 the first word after its last) and ``words`` (how many guard words changed on that side)."""
        if any(a.backing.is_cuda for a in self.allocations):
            _torch.cuda.synchronize()
        sides = [(a, side, g) for a in self.allocations for side, g in (('before', a.front), ('after', a.back))]
        if not sides:
            return []
        counts = _torch.stack([self._compare(g).sum() for _, _, g in sides]).cpu().tolist()
        out = []
        for (a, side, g), n in zip(sides, counts):
            if n:
                first = int(_torch.nonzero(self._compare(g))[0])
                out.append({'function': a.function, 'line': a.line, 'shape': a.shape, 'side': side,
                            'offset': 4 * (first - g.numel()) if side == 'before' else 4 * first, 'words': int(n)})
        return out

    def payload_bytes(self):
        return sum(a.nbytes for a in self.allocations)


class _Placement:
    """What hostile() remembers about one placed input: the backing buffer, where the view starts, the fill word, and how many words of the
    logical elements differ from that word (so that "every other word still holds the fill" is one count, without a second copy of the buffer)."""
    __slots__ = ('backing', 'first', 'word', 'other')


def _bits(t):
    return t.contiguous().view(_torch.int32) if t.element_size() == 4 else t.contiguous()


def hostile(t, fill, shift=0):
    """A tensor with ``t``'s shape, strides, dtype and values whose storage is a view into a buffer owned here,

        | guard (fill words) | payload: the bytes the view spans, fill between the logical elements | guard (fill words) |

    under the layout rules of this module: the payload starts ``shift`` bytes after a 512-byte boundary, the trailing guard at the first 4-byte
    word after the last byte the view spans, each guard at least the payload size and at least 64 KiB.  ``fill``: a key of ``FILLS``.  The
    result keeps the backing buffer alive (it is a view of it); ``hostile_changes(result, t)`` says whether any byte of the buffer -- logical
    elements, padding, guards -- was written since.  Elements of four bytes (what the kernels take)."""
    if fill not in FILLS:
        raise ValueError('fill must be one of %s, got %r' % (sorted(FILLS), fill))
    if t.element_size() != 4:
        raise ValueError('hostile() places tensors of 4-byte elements, got %s' % t.dtype)
    if shift < 0 or shift >= ALIGN or shift % 4:
        raise ValueError('shift must be a multiple of 4 in [0, %d), got %r' % (ALIGN, shift))
    shape, strides = tuple(t.shape), tuple(t.stride())
    nbytes = _storage_elems(shape, strides) * 4
    guard = max(MIN_GUARD, _round_up(nbytes, ALIGN))
    backing = _torch.empty((guard + ALIGN + shift + nbytes + guard) // 4, dtype=_torch.int32, device=t.device)
    first = _round_up(backing.data_ptr() + guard, ALIGN) - backing.data_ptr() + shift          # the view's first byte, from the backing buffer's first
    backing.fill_(FILLS[fill])
    out = _torch.as_strided(backing.view(_torch.uint8)[first:first + nbytes].view(t.dtype), shape, strides)
    out.copy_(t.detach())
    rec = _Placement()
    rec.backing, rec.first, rec.word = backing, first, FILLS[fill]
    rec.other = int((_bits(t.detach()) != rec.word).sum())
    out._hostile = rec
    return out


def hostile_changes(h, t):
    """None while every byte of the buffer behind ``h = hostile(t, ...)`` is as placed; else the byte offset, from the view's first byte, of the
    first changed word (negative: in front of it) and the number of changed words."""
    rec = h._hostile
    if _torch.equal(_bits(h), _bits(t.detach())) and int((rec.backing != rec.word).sum()) == rec.other:
        return None
    want = _torch.full_like(rec.backing, rec.word)          # (a failure only: the buffer once more)
    _torch.as_strided(want, tuple(t.shape), tuple(t.stride()), rec.first // 4).copy_(t.detach().view(_torch.int32))
    diff = rec.backing != want
    return {'offset': 4 * int(_torch.nonzero(diff)[0]) - rec.first, 'words': int(diff.sum())}


class _TorchProxy:
    """``torch`` for ``op/_backend.py``: every attribute is the real one except the three allocating calls."""

    def __init__(self, guard):
        object.__setattr__(self, '_guard', guard)
        for name in ('empty', 'empty_like', 'zeros'):
            object.__setattr__(self, name, getattr(guard, name))

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError('the torch proxy of tests/guarded_alloc.py is read-only')


@contextlib.contextmanager
def guarded(backend_module, poison='nan', canary=CANARY):
    """For the duration: ``backend_module.torch`` is the allocating proxy and ``HipBackend._launch`` records entry names.  Yields the ``Guard``;
    both are restored on exit, also after an exception.  ``canary``: the word of every guard (default ``CANARY``; ``POISONS['nan']`` or
    ``POISONS['big']`` surround every intermediate with that poison for the kernel that reads it next)."""
    guard = Guard(poison, canary)
    real_torch = backend_module.torch
    real_launch = backend_module.HipBackend._launch

    def recording_launch(self, dev, entry, *args, **kw):
        guard.entries.append(entry)
        return real_launch(self, dev, entry, *args, **kw)

    backend_module.torch = _TorchProxy(guard)
    backend_module.HipBackend._launch = recording_launch
    try:
        yield guard
    finally:
        backend_module.torch = real_torch
        backend_module.HipBackend._launch = real_launch
