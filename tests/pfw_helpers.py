"""Shared by the container tests (test_pfw_cpu.py, test_vadnet_cpu.py, test_punc_cpu.py): a packed `.pfw` with its header
re-serialised after an edit, and / or truncated."""
import json
import struct

from aliparaformerasr_amd import weights as W


def split(blob):
    """(header dict, offset of the data section) of a packed container"""
    hlen = struct.unpack_from("<Q", blob, 8)[0]
    return json.loads(bytes(blob[16:16 + hlen]).decode()), (16 + hlen + 255) // 256 * 256


def repack(cfg, w, edit_header=None, cut=None):
    blob = bytearray(W.pack_pfw(cfg, w))
    if edit_header:
        hdr, base = split(blob)
        data = bytes(blob[base:])
        edit_header(hdr)
        h2 = json.dumps(hdr).encode()
        pre = 16 + len(h2)
        blob = bytearray(b"PFW1" + struct.pack("<IQ", 1, len(h2)) + h2 + b"\0" * ((-pre) % 256) + data)
    if cut is not None:
        blob = blob[:cut]
    return bytes(blob)
