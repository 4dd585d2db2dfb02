"""The VR180 photo container without a GPU and without libxmp: ``assemble_vr180_photo`` / ``read_vr180_photo`` are inverses, Pillow
opens the result and decodes the left eye, every APP1 segment fits a JPEG segment, the extended chunks tile the packet and the GUID is
the packet's MD5 (Adobe XMP Specification Part 3); the CLI's new flags reach the functions behind them, and without them the commands
take the routes they took."""
import base64
import hashlib
import io
import struct

import numpy as np
import pytest

import jpg_cases as PC
import jpg_ref as R
import jpgdec_cases as JC

XMP_ID = b"http://ns.adobe.com/xap/1.0/\x00"
EXT_ID = b"http://ns.adobe.com/xmp/extension/\x00"


def _eyes(h, w, seed, quality=90, noise=False):
    make = PC.noise if noise else PC.smooth
    return JC.pillow(make(h, w, 3, seed), quality, "420"), JC.pillow(make(h, w, 3, seed + 1), quality, "420")


# a right eye small enough for one chunk, and one that needs at least three (base64 of more than 2 * 65400 * 3 / 4 bytes)
PAIRS = {"one_chunk": _eyes(32, 48, 600), "three_chunks": _eyes(256, 256, 602, 100, noise=True)}


def _app1(data):
    return [data[a + 4:e] for m, a, e in JC.header_segments(data) if m == 0xE1]


@pytest.mark.parametrize("name", list(PAIRS))
def test_read_is_the_inverse_of_assemble(name):
    from vr180_convert_amd import vr180_photo as P
    from vr180_convert_amd.calibration_cv import vr180_xmp_properties

    left, right = PAIRS[name]
    w, h = 2 * R.decode(left).shape[1], R.decode(left).shape[0]
    photo = P.assemble_vr180_photo(left, right, w, h)
    got_l, got_r, props = P.read_vr180_photo(photo)
    assert got_l == left and got_r == right
    assert props == vr180_xmp_properties(w, h)
    assert all(isinstance(v, (int, str)) for _, _, v in props)


@pytest.mark.parametrize("name", list(PAIRS))
def test_container_follows_the_specification(name):
    from PIL import Image

    from vr180_convert_amd import vr180_photo as P

    left, right = PAIRS[name]
    photo = P.assemble_vr180_photo(left, right, 512, 256)
    # Pillow opens it and decodes the left eye
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(photo)).convert("RGB")), np.asarray(Image.open(io.BytesIO(left)).convert("RGB")))
    segs = JC.header_segments(photo)
    assert [m for m, _, _ in segs][:2] == [0xE0, 0xE1]                          # behind APP0: the standard packet, then the chunks
    assert all(e - a - 2 <= 65535 for m, a, e in segs if m == 0xE1)             # the length field counts itself and the body
    bodies = _app1(photo)
    std = [b for b in bodies if b.startswith(XMP_ID)]
    ext = [b[len(EXT_ID):] for b in bodies if b.startswith(EXT_ID)]
    assert len(std) == 1 and len(ext) == len(bodies) - 1
    assert (len(ext) == 1) if name == "one_chunk" else (len(ext) >= 3)
    guids = {c[:32] for c in ext}
    totals = {struct.unpack(">I", c[32:36])[0] for c in ext}
    assert len(guids) == 1 and len(totals) == 1
    packet, at = b"", 0
    for c in ext:                                                               # in file order the offsets tile the packet
        assert struct.unpack(">I", c[36:40])[0] == at and 0 < len(c) - 40 <= 65400
        packet += c[40:]
        at += len(c) - 40
    assert at == totals.pop() == len(packet)
    guid = guids.pop().decode()
    assert guid == hashlib.md5(packet).hexdigest().upper() and guid != "06A56CB0A1A7FAFDA459CA3FAA14B474"
    assert f'xmpNote:HasExtendedXMP="{guid}"'.encode() in std[0] and b'GImage:Mime="image/jpeg"' in std[0]
    assert std[0][len(XMP_ID):].startswith(b"<?xpacket begin=") and std[0].rstrip().endswith(b'<?xpacket end="w"?>')
    assert b'GPano:ProjectionType="equirectangular"' in std[0] and b'GPano:FullPanoWidthPixels="512"' in std[0]
    assert base64.b64encode(right) in packet and packet.startswith(b"<x:xmpmeta")


def test_files_without_app0_and_damaged_containers():
    from vr180_convert_amd import vr180_photo as P

    left, right = PAIRS["one_chunk"]
    bare = JC.without(left, 0xE0)
    photo = P.assemble_vr180_photo(bare, right, 96, 32)
    assert JC.header_segments(photo)[0][0] == 0xE1 and P.read_vr180_photo(photo)[:2] == (bare, right)
    with pytest.raises(ValueError, match="SOI"):
        P.assemble_vr180_photo(b"PNG" + left, right, 96, 32)
    with pytest.raises(ValueError, match="SOI"):
        P.assemble_vr180_photo(left, b"", 96, 32)
    with pytest.raises(ValueError, match="no XMP"):
        P.read_vr180_photo(left)
    good = P.assemble_vr180_photo(*PAIRS["three_chunks"], 512, 256)
    segs = [(m, a, e) for m, a, e in JC.header_segments(good) if m == 0xE1]
    m, a, e = segs[2]
    with pytest.raises(ValueError, match="tile"):
        P.read_vr180_photo(good[:a] + good[e:])                      # a chunk is missing
    flipped = bytearray(good)
    flipped[e - 10] ^= 1
    with pytest.raises(ValueError, match="MD5"):
        P.read_vr180_photo(bytes(flipped))
    # element form, as other writers serialise XMP: read all the same
    props = P._properties(b'<x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="http://www.w3.org/1999/02/22-rdf-syntax-ns#">'
                          b'<rdf:Description rdf:about="" xmlns:GPano="http://ns.google.com/photos/1.0/panorama/">'
                          b"<GPano:PoseRollDegrees>0</GPano:PoseRollDegrees></rdf:Description></rdf:RDF></x:xmpmeta>")
    assert props == [("http://ns.google.com/photos/1.0/panorama/", "PoseRollDegrees", "0")]


# ---- plumbing: the new flags reach the new functions, and nothing changes without them -------------------------------------------------
def test_cli_flags_reach_the_transcoder_and_keep_the_old_route(tmp_path, monkeypatch):
    from PIL import Image
    from typer.testing import CliRunner

    from vr180_convert_amd import _io, cli, jpeg_transcode_device as T, vr180_photo as P

    left, right = PAIRS["one_chunk"]
    sbs = tmp_path / "sbs.jpg"
    sbs.write_bytes(left)
    calls = []
    monkeypatch.setattr(T, "swap_sbs_jpeg", lambda p, **k: calls.append(("swap", p)) or b"SWAPPED")
    monkeypatch.setattr(T, "split_sbs_jpeg", lambda p, **k: calls.append(("split", p)) or (left, right))
    run = CliRunner()
    r = run.invoke(cli.app, ["swap", "--lossless", "--no-overwrite", str(sbs)])
    assert r.exit_code == 0, r.output
    assert calls == [("swap", left)] and (tmp_path / "sbs.swap.jpg").read_bytes() == b"SWAPPED" and sbs.read_bytes() == left
    r = run.invoke(cli.app, ["xmp", "--device", str(sbs)])
    assert r.exit_code == 0, r.output
    out = tmp_path / "sbs.xmp.jpg"
    got = P.read_vr180_photo(out.read_bytes())
    assert calls[-1] == ("split", left) and got[:2] == (left, right)
    assert dict((n, v) for _, n, v in got[2])["FullPanoWidthPixels"] == 48 and dict((n, v) for _, n, v in got[2])["FullPanoHeightPixels"] == 32

    # a file the transcoder does not take: the command says so and keeps its existing route
    def refuse(p, **k):
        raise ValueError("half of the width is no multiple of the MCU width")

    monkeypatch.setattr(T, "swap_sbs_jpeg", refuse)
    written = []
    monkeypatch.setattr(_io, "imwrite", lambda p, im: written.append((p, im.shape)))
    r = run.invoke(cli.app, ["swap", "--lossless", str(sbs)])
    assert r.exit_code == 0 and written == [(sbs, (32, 48, 3))]
    # without the flag, and for other formats with it, the transcoder is not asked
    monkeypatch.setattr(T, "swap_sbs_jpeg", lambda *a, **k: pytest.fail("asked without --lossless"))
    assert run.invoke(cli.app, ["swap", str(sbs)]).exit_code == 0 and len(written) == 2
    png = tmp_path / "sbs.png"
    Image.fromarray(np.zeros((8, 16, 3), np.uint8)).save(png)
    assert run.invoke(cli.app, ["swap", "--lossless", str(png)]).exit_code == 0 and written[-1] == (png, (8, 16, 3))


def test_apply_lr_vr180_argument_rules():
    import vr180_convert_amd as V
    from vr180_convert_amd.transformer import EquirectangularEncoder, FisheyeDecoder

    t = EquirectangularEncoder() * FisheyeDecoder("equidistant")
    img = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="merge"):
        V.apply_lr(t, left_path=img, right_path=img, out_path="x.jpg", merge=True, device_jpeg="vr180")
    with pytest.raises(ValueError, match="out_path"):  # before anything is remapped, device_png or not
        V.apply_lr(t, left_path=img, right_path=img, out_path="x.png", device_jpeg="vr180", device_png=True)
    with pytest.raises(ValueError, match="device_jpeg"):
        V.apply(t, in_paths=[img], out_paths=["x.jpg"], device_jpeg="vr180")
    with pytest.raises(ValueError, match="device_jpeg"):
        V.apply_lr(t, left_path=img, right_path=img, out_path="x.jpg", device_jpeg="vr181")
