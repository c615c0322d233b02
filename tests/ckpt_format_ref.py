"""An independent restatement of the checkpoint file's framing for tests/test_ckpt_format.py,
tests/test_abi_checkpoint_ex.py and tests/test_gpu_checkpoint_observers.py, written from the format comments of
csrc/ckpt_format.h and csrc/iblb_ctx.hip, not from their code.

A file is the fluid part, then nothing, or sections closed by the end section.  A section: an 8-byte tag, the
payload's length as a little-endian int64, the payload.  Tags in the only order allowed, each at most once:
IBLBSCL1, IBLBTRC1, IBLBAVG1, IBLBEND1; the end section's payload is empty and nothing follows it."""
import struct

TAGS = (b"IBLBSCL1", b"IBLBTRC1", b"IBLBAVG1", b"IBLBEND1")
SCALAR, TRACERS, AVERAGE, END = range(4)
BITS = (1, 2, 4)  # IBLB_CKPT_SCALAR, _TRACERS, _AVERAGE
# the scanner's verdicts, in the order of ckpt_format.h's ScanStatus
OK, IO, FLUID_SHORT, HEADER_SHORT, TAG, ORDER, LENGTH, NO_END, TRAILING = range(9)

MAGIC = b"IBLBCK01"
HEADER_BYTES = 8 + 12 * 8 + 6 * 8


def fluid_part(nx, ny, prec=0, t=0, ns=0, cilia=0, c_num=0, ncol=None, x_begin=0, tau=0.8, tau2=1.0, pops=None):
    """A fluid part as iblb_save_checkpoint writes it: magic, 12 int64 (version 1, nx, ny, x_begin, ncol, precision,
    step, points, cilia on, c_num, T, p_step), 6 doubles (Q, c_space, tau, tau2, gx, gy), nine planes of ncol * ny
    populations in the storage precision (zeros unless given), per point two float pairs and an int, and with cilia
    7 floats per filament sample (9600 per cilium) and 5 per boundary point (96 per cilium)."""
    ncol = nx if ncol is None else ncol
    head = MAGIC + struct.pack("<12q", 1, nx, ny, x_begin, ncol, prec, t, ns, cilia, c_num, 0, 0)
    head += struct.pack("<6d", 0.0, 0.0, tau, tau2, 0.0, 0.0)
    body = bytes(9 * ncol * ny * (8 if prec == 0 else 4)) if pops is None else pops
    body += bytes(20 * ns)
    if cilia:
        body += bytes(4 * (7 * 9600 + 5 * 96) * c_num)
    return head + body


def section(kind, payload=b"", length=None, tag=None):
    return (TAGS[kind] if tag is None else tag) + struct.pack("<q", len(payload) if length is None else length) + payload


def scan(data: bytes, fluid_end: int):
    """(verdict, {kind: (payload offset, payload length)}) of a file's bytes; the dictionary is empty unless OK."""
    size = len(data)
    if size < fluid_end:
        return FLUID_SHORT, {}
    pos, last, found = fluid_end, -1, {}
    while pos < size:
        if size - pos < 16:
            return HEADER_SHORT, {}
        tag, (length,) = data[pos:pos + 8], struct.unpack("<q", data[pos + 8:pos + 16])
        if tag not in TAGS:
            return TAG, {}
        kind = TAGS.index(tag)
        if kind <= last:
            return ORDER, {}
        pos += 16
        if length < 0 or length > size - pos or (kind == END and length != 0):
            return LENGTH, {}
        found[kind] = (pos, length)
        pos += length
        last = kind
        if kind == END:
            return (OK, found) if pos == size else (TRAILING, {})
    return (OK, {}) if last < 0 else (NO_END, {})


def observers(found) -> int:
    return sum(BITS[k] for k in found if k != END)
