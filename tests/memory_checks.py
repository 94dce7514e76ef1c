"""Shared pieces of the memory-contract tests (tests/test_gpu_memory_contract.py on the device,
tests/test_memory_checks_host.py for the CPU half): what a call of include/nhans_hip.h does to the memory BESIDE the ranges
it documents.  The rule under test: a call writes the counted elements of each clip's room and nothing else of the caller's
memory, and reads no element outside the ranges its offsets name.  head_checks.guarded / canary_damage, generalised.

Guarded outputs.  A buffer is GUARD sentinel words, the region handed to the library, GUARD sentinel words; the region is
sentinel too, the slack between a clip's count and its room included.  After the call `findings` lists guard words that
changed (the first one and its distance from the region), slack elements that changed and elements of a documented range
that still hold the sentinel (holes).  Which elements are documented is a boolean mask over the region (`prefix_mask` for
the usual "first count elements of every room").  A legitimate output may equal a sentinel (an int16 has 65,536 values): a
case is run with two different sentinels and an element is a hole only if it equals the sentinel in BOTH runs.
    What this cannot see: a stray store further than GUARD 32-bit words (1 KiB) from the region lands outside the buffer;
a stray store that writes the sentinel's own bits; a stray LOAD whose value does not reach an output.

Surrounded inputs.  The same pieces are laid out twice with identical bits inside every documented range and different
bits everywhere else -- before the first piece, in the gaps, behind the last: zeros (variant "A") or poison (variant "B":
NaN for float32 samples, 1e30 for log-magnitude rows -- expf makes it inf, which a max cannot hide as it hides NaN --,
alternating 32767 / -32768 for int16).  A call that reads only what its offsets name gives the same bits for both.

Alignment.  Both place the first element of the region at element offset `align` from a 16-byte boundary (0..3 for
float32, 0..7 for int16, 0..1 for float64); `ragged_offsets` then walks the clips' starts through every phase.
"""
import collections

import numpy as np
import torch

GUARD = 256                     # 32-bit words either side, head_checks.GUARD
# kind: (numpy element type, numpy integer type of the same width)
KINDS = {"f32": (np.float32, np.int32), "i16": (np.int16, np.int16), "f64": (np.float64, np.int64)}
# two bit patterns per kind.  float32: 3.5e13 and a NaN; float64: 1.7e130 and a NaN; int16: 23294 and 15373
SENTINELS = {"f32": (0x5AFEC0DE, 0x7FD5AFE5), "i16": (0x5AFE, 0x3C0D), "f64": (0x5AFEC0DE5AFEC0DE, 0x7FF5AFE55AFEC0DE)}
POISON = ("nan", "big", "pcm")

Finding = collections.namedtuple("Finding", "what count first clip text")   # what: guard_before | guard_after | slack | hole


def itemsize(kind):
    return np.dtype(KINDS[kind][0]).itemsize


def lanes(kind):
    """Elements per 16 bytes."""
    return 16 // itemsize(kind)


def guard_elements(kind):
    return GUARD * 4 // itemsize(kind)


def ragged_offsets(counts, kind="f32", tail=3):
    """Region-relative offsets [n + 1] with room >= count + 1 for every clip (odd gaps of 1 .. lanes elements) such that clip c
    starts at phase c mod lanes of the region's own phase: with `align` the clips walk through every 16-byte phase."""
    la, off = lanes(kind), [0]
    for c, n in enumerate(counts):
        end = off[-1] + int(n) + 1
        if c + 1 < len(counts):
            end += ((c + 1) - end) % la
        else:
            end += tail - 1
        off.append(end)
    return off


def tight_offsets(counts):
    return [0] + [int(v) for v in np.cumsum(np.asarray(counts, dtype=np.int64))]


def prefix_mask(offsets, counts):
    """The documented elements of a region of offsets[-1] elements: the first counts[c] of room c."""
    m = np.zeros(int(offsets[-1]), dtype=bool)
    for c, n in enumerate(counts):
        assert 0 <= n <= offsets[c + 1] - offsets[c], "clip %d: count %d, room %d" % (c, n, offsets[c + 1] - offsets[c])
        m[offsets[c]:offsets[c] + int(n)] = True
    return m


class _Buffer:
    """front elements, `size` region elements, back elements as one tensor of the kind's integer type; the region's first
    element sits `align` elements behind a 16-byte boundary."""

    def __init__(self, kind, size, align, host, device):
        self.kind, self.size, self.align = kind, int(size), int(align)
        assert 0 <= align < lanes(kind)
        assert len(host) == self.front + self.size + self.back
        self.bits = torch.from_numpy(host).to(device)
        assert self.bits.data_ptr() % 16 == 0
        self.ptr = self.bits.data_ptr() + self.front * itemsize(kind)
        assert self.ptr % 16 == align * itemsize(kind)

    @property
    def front(self):
        return guard_elements(self.kind) + self.align

    @property
    def back(self):
        return guard_elements(self.kind)

    def host_bits(self):
        return self.bits.detach().cpu().numpy()

    def region_bits(self):
        return self.host_bits()[self.front:self.front + self.size]

    def region(self):
        """The region as the kind's own element type (a host copy)."""
        return self.region_bits().view(KINDS[self.kind][0])

    def element_ptr(self, i):
        """Address of region element i (for calls that take a pointer per piece)."""
        assert 0 <= i <= self.size
        return self.ptr + int(i) * itemsize(self.kind)


def _empty(kind, size, align, value):
    n = guard_elements(kind) + align + int(size) + guard_elements(kind)
    return np.full(n, value, dtype=KINDS[kind][1])


class Guarded(_Buffer):
    """An output buffer, every element the sentinel `which` (0 or 1) of its kind."""

    def __init__(self, kind, size, align=0, which=0, device="cpu"):
        self.sentinel = SENTINELS[kind][which]
        super().__init__(kind, size, align, _empty(kind, size, align, self.sentinel), device)

    def place(self, start, values):
        """Writes input values into the region (in-place calls: the input lives inside the guarded buffer)."""
        v = np.ascontiguousarray(values, dtype=KINDS[self.kind][0]).view(KINDS[self.kind][1])
        assert 0 <= start and start + len(v) <= self.size
        self.bits[self.front + start:self.front + start + len(v)] = torch.from_numpy(v).to(self.bits.device)


def findings(runs, mask, offsets=None):
    """runs: one Guarded after its call, or several of the same geometry filled with different sentinels after the same
    call; mask: bool [size], True where the call documents a store.  -> list of Finding (empty: every guard word and slack
    element intact in every run, every documented element written).  offsets: names the clip of a slack element / hole."""
    runs = [runs] if isinstance(runs, Guarded) else list(runs)
    mask = np.asarray(mask, dtype=bool)
    out, never = [], None
    words = lambda g, elements: -(-elements * itemsize(g.kind) // 4)

    def clip_of(i):
        if offsets is None:
            return None
        c = int(np.searchsorted(np.asarray(offsets), i, side="right")) - 1
        return min(max(c, 0), len(offsets) - 2)

    for k, g in enumerate(runs):
        assert g.size == len(mask) and g.kind == runs[0].kind
        w = g.host_bits()
        s = np.array(g.sentinel, dtype=w.dtype)
        bad = np.flatnonzero(w[:g.front] != s)
        if len(bad):
            first = int(bad[-1])                                  # the one nearest to the region
            out.append(Finding("guard_before", len(bad), first - g.front, None,
                               "run %d: %d guard elements before the region overwritten, nearest %d words before it (0x%x)"
                               % (k, len(bad), words(g, g.front - first), int(w[first]) & (2 ** (8 * w.itemsize) - 1))))
        tail = w[g.front + g.size:]
        bad = np.flatnonzero(tail != s)
        if len(bad):
            first = int(bad[0])
            out.append(Finding("guard_after", len(bad), first, None,
                               "run %d: %d guard elements after the region overwritten, first %d words behind it (0x%x)"
                               % (k, len(bad), words(g, first + 1), int(tail[first]) & (2 ** (8 * w.itemsize) - 1))))
        reg = w[g.front:g.front + g.size]
        bad = np.flatnonzero((reg != s) & ~mask)
        if len(bad):
            first = int(bad[0])
            out.append(Finding("slack", len(bad), first, clip_of(first),
                               "run %d: %d slack elements written, first at region element %d (clip %s)"
                               % (k, len(bad), first, clip_of(first))))
        same = (reg == s) & mask
        never = same if never is None else (never & same)
    bad = np.flatnonzero(never)
    if len(bad):
        first = int(bad[0])
        out.append(Finding("hole", len(bad), first, clip_of(first),
                           "%d documented elements never written, first at region element %d (clip %s)"
                           % (len(bad), first, clip_of(first))))
    return out


def report(fs):
    return "; ".join(f.text for f in fs)


def poison_values(kind, poison, n, phase=0):
    """n poison elements as the kind's integer bits; `phase`: the absolute index of the first (the int16 pattern alternates)."""
    ft, it = KINDS[kind]
    if poison == "nan":
        assert kind == "f32"
        v = np.full(n, np.nan, dtype=ft)
    elif poison == "big":
        assert kind == "f32"
        v = np.full(n, 1e30, dtype=ft)
    else:
        assert poison == "pcm" and kind == "i16"
        v = np.where((np.arange(n) + phase) % 2 == 0, 32767, -32768).astype(ft)
    return v.view(it)


class Surrounded(_Buffer):
    """An input buffer: pieces[i] at region element starts[i] (ascending, not overlapping), every other element -- GUARD words
    before, the gaps, GUARD words behind -- zero (variant "A") or poison (variant "B")."""

    def __init__(self, kind, pieces, starts, size=None, align=0, variant="A", poison=None, device="cpu"):
        ft, it = KINDS[kind]
        assert variant in ("A", "B") and len(pieces) == len(starts)
        size = int(size if size is not None else (starts[-1] + len(pieces[-1]) if len(pieces) else 0))
        host = _empty(kind, size, align, 0)
        if variant == "B":
            poison = poison or ("pcm" if kind == "i16" else "nan")
            host[:] = poison_values(kind, poison, len(host))
        front = guard_elements(kind) + align
        self.inside = np.zeros(len(host), dtype=bool)
        end = 0
        for p, s in zip(pieces, starts):
            p = np.ascontiguousarray(p, dtype=ft).reshape(-1)
            assert end <= s and s + len(p) <= size
            host[front + s:front + s + len(p)] = p.view(it)
            self.inside[front + s:front + s + len(p)] = True
            end = s + len(p)
        super().__init__(kind, size, align, host, device)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
