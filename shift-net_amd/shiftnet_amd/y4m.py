"""YUV4MPEG2 (Y4M) streams: the one video container that needs no codec.  Pure Python + numpy, no GPU.

A stream is one header line ``YUV4MPEG2 W<w> H<h> F<n>:<d> I<p|t|b|m> A<n>:<d> C<mode> X...`` and, per frame, a line ``FRAME[ params]``
followed by the planar payload: the Y plane, then U, then V (chroma planes ``ceil(W/2) x ceil(H/2)`` for 4:2:0), one byte per sample at
8 bit and one little-endian 16-bit word at 10 bit.  The reader needs ``read`` only, so it works on a pipe.

Supported chroma modes and how the device kernels (csrc/sn_yuv.hip) see them:
    420jpeg          4:2:0, chroma sited at the centre of the 2x2 block
    420mpeg2, 420    4:2:0, chroma sited on the left luma column, between the two rows
    420paldv         treated as 420mpeg2: its horizontal siting is the same, its alternating vertical siting is NOT modelled
    444              4:4:4
    420p10, 444p10   10 bit (420p10 is left-sited like 420mpeg2)
Interlaced streams and every other mode are refused.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import BinaryIO, Iterator, List, Optional

import numpy as np

MAGIC = b"YUV4MPEG2"
# mode -> (bits, chroma) with chroma 0 = 4:4:4, 1 = 4:2:0 centre-sited, 2 = 4:2:0 left-sited (the codes of sn_yuv_fmt)
MODES = {"420jpeg": (8, 1), "420mpeg2": (8, 2), "420": (8, 2), "420paldv": (8, 2), "444": (8, 0), "420p10": (10, 2), "444p10": (10, 0)}


class Y4MError(ValueError):
    pass


@dataclass
class Y4MHeader:
    width: int
    height: int
    fps: str = "25:1"
    interlace: str = "p"
    aspect: str = "0:0"
    chroma: str = "420jpeg"          # the C tag; a stream without one is 420jpeg (the format's default)
    extensions: List[str] = field(default_factory=list)     # X tags, without the X

    @property
    def bits(self) -> int:
        return MODES[self.chroma][0]

    @property
    def chroma_code(self) -> int:
        return MODES[self.chroma][1]

    @property
    def color_range(self) -> Optional[str]:
        """'full' / 'limited' from XCOLORRANGE, None if the stream does not say."""
        for x in self.extensions:
            if x.upper().startswith("COLORRANGE="):
                return x.split("=", 1)[1].lower()
        return None

    @property
    def frame_bytes(self) -> int:
        h, w = self.height, self.width
        c = h * w if self.chroma_code == 0 else ((h + 1) // 2) * ((w + 1) // 2)
        return (h * w + 2 * c) * (1 if self.bits == 8 else 2)

    def line(self) -> bytes:
        tags = [f"W{self.width}", f"H{self.height}", f"F{self.fps}", f"I{self.interlace}", f"A{self.aspect}", f"C{self.chroma}"]
        tags += ["X" + x for x in self.extensions]
        return MAGIC + b" " + " ".join(tags).encode("ascii") + b"\n"


def output_header(header: Y4MHeader, out_format: Optional[str] = None) -> Y4MHeader:
    """The header of the stream the restorer writes for ``header``'s: the new C tag (``out_format``, a key of MODES; None keeps the input's), every
    other tag and every X extension the input's."""
    if out_format is None:
        return header
    if out_format not in MODES:
        raise Y4MError(f"Y4M: output format C{out_format} is not supported (supported: {', '.join('C' + m for m in MODES)})")
    return replace(header, chroma=out_format, extensions=list(header.extensions))


def _read_exact(f: BinaryIO, n: int) -> bytes:
    """n bytes, fewer only at end of stream (a pipe may return short reads)."""
    chunks, got = [], 0
    while got < n:
        b = f.read(n - got)
        if not b:
            break
        chunks.append(b)
        got += len(b)
    return chunks[0] if len(chunks) == 1 else b"".join(chunks)


def _read_line(f: BinaryIO, limit: int = 4096) -> bytes:
    out = bytearray()
    while len(out) < limit:
        b = f.read(1)
        if not b or b == b"\n":
            return bytes(out)
        out += b
    raise Y4MError("Y4M: header line longer than %d bytes" % limit)


def parse_header(line: bytes) -> Y4MHeader:
    parts = line.decode("ascii", "replace").split()
    if not parts or parts[0] != MAGIC.decode():
        raise Y4MError("not a YUV4MPEG2 stream (header %r)" % line[:32])
    h = Y4MHeader(0, 0)
    for p in parts[1:]:
        tag, val = p[0], p[1:]
        if tag == "W":
            h.width = int(val)
        elif tag == "H":
            h.height = int(val)
        elif tag == "F":
            h.fps = val
        elif tag == "I":
            h.interlace = val
        elif tag == "A":
            h.aspect = val
        elif tag == "C":
            h.chroma = val
        elif tag == "X":
            h.extensions.append(val)
    if h.width < 1 or h.height < 1:
        raise Y4MError("Y4M: missing or bad W / H in %r" % line)
    if h.interlace not in ("p", "?"):
        raise Y4MError(f"Y4M: interlaced stream (I{h.interlace}) is not supported; deinterlace first")
    if h.chroma not in MODES:
        raise Y4MError(f"Y4M: chroma mode C{h.chroma} is not supported (supported: {', '.join('C' + m for m in MODES)})")
    return h


class Y4MReader:
    """Iterate over the raw frame payloads (``uint8`` arrays of ``header.frame_bytes``) of a Y4M stream; ``fileobj`` needs ``read`` only."""

    def __init__(self, fileobj: BinaryIO) -> None:
        self.f = fileobj
        self.header = parse_header(_read_line(fileobj))

    def read_into(self, buf: np.ndarray) -> bool:
        """The next payload into ``buf`` (uint8, frame_bytes); False at the end of the stream."""
        line = _read_line(self.f)
        if not line:
            return False
        if not line.startswith(b"FRAME"):
            raise Y4MError("Y4M: expected FRAME, got %r" % line[:32])
        n = self.header.frame_bytes
        data = _read_exact(self.f, n)
        if len(data) != n:
            raise Y4MError(f"Y4M: truncated frame ({len(data)} of {n} bytes)")
        buf[:n] = np.frombuffer(data, np.uint8)
        return True

    def __iter__(self) -> Iterator[np.ndarray]:
        while True:
            buf = np.empty(self.header.frame_bytes, np.uint8)
            if not self.read_into(buf):
                return
            yield buf


class Y4MWriter:
    def __init__(self, fileobj: BinaryIO, header: Y4MHeader) -> None:
        self.f, self.header = fileobj, header
        fileobj.write(header.line())

    def write(self, payload) -> None:
        payload = np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1)
        if payload.size != self.header.frame_bytes:
            raise Y4MError(f"Y4M: payload of {payload.size} bytes, the header says {self.header.frame_bytes}")
        self.f.write(b"FRAME\n")
        self.f.write(memoryview(payload))
