"""Google VR180 photo files without libxmp / exempi / OpenCV: the left eye is the JPEG a plain viewer shows, the right eye rides in
its XMP metadata, and a headset or Google Photos shows the two in stereo.  Host code only; the eyes come as JPEG bytes -- from
``split_sbs_jpeg`` (a side-by-side file cut without a JPEG generation) or from ``encode_jpeg_tensors`` (a device result).

The container (Adobe XMP Specification Part 3, "Extended XMP in JPEG"; Google's GPano / GImage namespaces):

* one standard XMP segment, APP1 with the identifier ``http://ns.adobe.com/xap/1.0/\\0``: the GPano properties of
  ``calibration_cv.vr180_xmp_properties``, ``GImage:Mime = image/jpeg`` and ``xmpNote:HasExtendedXMP``, the GUID of the extended packet;
* the extended packet, which carries ``GImage:Data`` -- the right eye in base64 --, cut into APP1 segments with the identifier
  ``http://ns.adobe.com/xmp/extension/\\0``, each with the GUID (32 characters), the packet's length and the chunk's offset as
  big-endian ``uint32`` and at most 65 400 bytes of the packet.  The GUID is the upper-case hexadecimal MD5 of the packet.

Both kinds of segment go behind the file's APP0, in that order; nothing else of the left eye's file changes.  INTEGRATION.md section 9
has the contract."""
from __future__ import annotations

import base64
import hashlib
import struct
import xml.etree.ElementTree as ET
from pathlib import Path
from typing import Any
from xml.sax.saxutils import quoteattr

from .calibration_cv import XMP_GIMAGE, XMP_GPANO, XMP_NOTE, vr180_xmp_properties

XMP_ID = b"http://ns.adobe.com/xap/1.0/\x00"
XMP_EXT_ID = b"http://ns.adobe.com/xmp/extension/\x00"
CHUNK = 65400                                   # bytes of the extended packet per segment
_RDF = "http://www.w3.org/1999/02/22-rdf-syntax-ns#"
_PREFIX = {XMP_GPANO: "GPano", XMP_GIMAGE: "GImage", XMP_NOTE: "xmpNote"}


def _text(value: Any) -> str:
    """a property's text: strings as they are, numbers as integers (the reference writes them with set_property_int)"""
    return value if isinstance(value, str) else str(int(value))


def _description(props: list) -> str:
    """one rdf:Description with the properties as attributes"""
    spaces = "".join(f' xmlns:{_PREFIX[ns]}="{ns}"' for ns in dict.fromkeys(ns for ns, _, _ in props))
    attrs = "".join(f" {_PREFIX[ns]}:{name}={quoteattr(_text(v))}" for ns, name, v in props)
    return (f'<x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="{_RDF}"><rdf:Description rdf:about=""{spaces}{attrs}/>'
            "</rdf:RDF></x:xmpmeta>")


def _segment(marker: int, body: bytes) -> bytes:
    if len(body) > 65533:
        raise ValueError("a JPEG segment holds at most 65533 bytes")
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def _segments(data: bytes):
    """(marker, first byte, byte behind) of every segment behind SOI up to and including SOS; ``ValueError`` for anything else"""
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file: no SOI")
    pos = 2
    while True:
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise ValueError(f"not a JPEG file: marker expected at byte {pos}")
        if data[pos + 1] == 0xFF:  # a fill byte
            pos += 1
            continue
        m = data[pos + 1]
        end = pos + 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if end > len(data) or end < pos + 4:
            raise ValueError(f"not a JPEG file: the segment at byte {pos} leaves it")
        yield m, pos, end
        if m == 0xDA:
            return
        pos = end


def assemble_vr180_photo(left_jpeg: bytes, right_jpeg: bytes, width: int, height: int) -> bytes:
    """The VR180 photo of two eyes: ``left_jpeg`` with the XMP segments behind its APP0 (behind SOI where it has none).  ``width`` and
    ``height``: of the side-by-side image the eyes are the halves of -- what ``vr180_xmp_properties`` takes."""
    left_jpeg, right_jpeg = bytes(left_jpeg), bytes(right_jpeg)
    first = next(_segments(left_jpeg))
    if right_jpeg[:2] != b"\xff\xd8":
        raise ValueError("the right eye is not a JPEG file: no SOI")
    extended = _description([(XMP_GIMAGE, "Data", base64.b64encode(right_jpeg).decode("ascii"))]).encode("utf-8")
    guid = hashlib.md5(extended).hexdigest().upper()  # noqa: S324 - the specification's GUID, not a secret
    props = vr180_xmp_properties(int(width), int(height)) + [(XMP_GIMAGE, "Mime", "image/jpeg"), (XMP_NOTE, "HasExtendedXMP", guid)]
    packet = ('<?xpacket begin="\ufeff" id="W5M0MpCehiHzreSzNTczkc9d"?>' + _description(props) + '<?xpacket end="w"?>').encode("utf-8")
    segs = [_segment(0xE1, XMP_ID + packet)]
    for at in range(0, len(extended), CHUNK):
        segs.append(_segment(0xE1, XMP_EXT_ID + guid.encode("ascii") + struct.pack(">II", len(extended), at) + extended[at:at + CHUNK]))
    cut = first[2] if first[0] == 0xE0 else 2
    return left_jpeg[:cut] + b"".join(segs) + left_jpeg[cut:]


def _properties(packet: bytes) -> list:
    """(namespace, name, text) of every property of a packet's rdf:Description elements, attributes and simple child elements alike"""
    text = packet.decode("utf-8")
    a, b = text.find("<x:xmpmeta"), text.rfind("</x:xmpmeta>")
    if a < 0 or b < 0:
        raise ValueError("no x:xmpmeta element in the XMP packet")
    root = ET.fromstring(text[a:b + len("</x:xmpmeta>")])  # noqa: S314 - no entities are declared in an XMP packet we accept
    out = []
    for d in root.iter(f"{{{_RDF}}}Description"):
        for key, value in d.attrib.items():
            ns, _, name = key[1:].partition("}")
            if key.startswith("{") and ns != _RDF:
                out.append((ns, name, value))
        for child in d:
            ns, _, name = child.tag[1:].partition("}")
            out.append((ns, name, child.text or ""))
    return out


def _value(text: str) -> Any:
    try:
        return int(text)
    except ValueError:
        return text


def read_vr180_photo(data: bytes) -> tuple[bytes, bytes, list]:
    """``(left_jpeg, right_jpeg, properties)`` of a VR180 photo: the file without its XMP segments, the embedded right eye, and the
    ``(namespace, name, value)`` of its GPano properties in the file's order, numbers as ``int`` -- for a file of
    ``assemble_vr180_photo(l, r, w, h)``: ``l``, ``r`` and what ``vr180_xmp_properties(w, h)`` lists.  ``ValueError`` where the file
    holds no such metadata, chunks are missing or overlap, or the GUID is not the extended packet's MD5."""
    data = bytes(data)
    standard, chunks, keep, at = None, [], [data[:2]], 2
    for m, a, e in _segments(data):
        keep.append(data[at:a])  # (fill bytes in front of a marker stay with the file)
        at = e
        body = data[a + 4:e]
        if m == 0xE1 and body.startswith(XMP_ID):
            standard = body[len(XMP_ID):]
        elif m == 0xE1 and body.startswith(XMP_EXT_ID):
            head = body[len(XMP_EXT_ID):]
            if len(head) < 40:
                raise ValueError("an extended XMP segment is shorter than its header")
            total, offset = struct.unpack(">II", head[32:40])
            chunks.append((head[:32].decode("ascii", "replace"), total, offset, head[40:]))
        else:
            keep.append(data[a:e])
    keep.append(data[at:])
    if standard is None:
        raise ValueError("no XMP segment: not a VR180 photo")
    props = _properties(standard)
    guid = next((v for ns, n, v in props if (ns, n) == (XMP_NOTE, "HasExtendedXMP")), None)
    if guid is None:
        raise ValueError("the XMP names no extended packet: not a VR180 photo")
    mine = sorted((c for c in chunks if c[0] == guid), key=lambda c: c[2])
    if not mine:
        raise ValueError(f"no extended XMP segment carries the GUID {guid}")
    total, packet = mine[0][1], b""
    for _, t, offset, part in mine:
        if t != total or offset != len(packet):
            raise ValueError("the extended XMP chunks do not tile the packet")
        packet += part
    if len(packet) != total:
        raise ValueError("the extended XMP packet is incomplete")
    if hashlib.md5(packet).hexdigest().upper() != guid:  # noqa: S324
        raise ValueError("the GUID is not the extended packet's MD5")
    b64 = next((v for ns, n, v in _properties(packet) if (ns, n) == (XMP_GIMAGE, "Data")), None)
    if b64 is None:
        raise ValueError("the extended packet carries no GImage:Data")
    return b"".join(keep), base64.b64decode(b64), [(ns, n, _value(v)) for ns, n, v in props if ns == XMP_GPANO]


def imwrite_vr180_tensor(path: Any, sbs_tensor: Any, **jpeg_kw: Any) -> None:
    """A device side-by-side result ``(H, W[, C])`` as a VR180 photo: the two halves are encoded on the device as one batch
    (``encode_jpeg_tensors``; ``jpeg_kw``: its ``quality``, ``subsampling``, ``restart_mcus``, ``optimize``) and assembled here.
    ``ValueError`` for an odd width."""
    from .jpeg_device import encode_jpeg_tensors

    h, w = int(sbs_tensor.shape[0]), int(sbs_tensor.shape[1])
    if w % 2:
        raise ValueError(f"a side-by-side image has an even width, not {w}")
    left, right = encode_jpeg_tensors([sbs_tensor[:, :w // 2], sbs_tensor[:, w // 2:]], **jpeg_kw)
    Path(path).write_bytes(assemble_vr180_photo(left, right, w, h))


__all__ = ["assemble_vr180_photo", "read_vr180_photo", "imwrite_vr180_tensor"]
