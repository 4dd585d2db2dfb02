"""The lossless JPEG composer on the MI355X: every case of tests/jpgxf_cases.py through ``v1c_jpeg_compose`` against the restatement
(jpgxf_ref.py), byte for byte, header and scan, at the default subsequence size and at 256 bits on a stream of its own; a damaged second
source, out-of-range coefficients and the refusal under stream capture; one source with transform 0 against ``v1c_jpeg_transcode``,
field by field; the Python entries ``transform_jpeg``, ``join_sbs_jpeg``,
``sbs_from_vr180_photo`` and ``normalize_orientation_jpeg``; and ``join`` on the command line, behind ``xmp --device`` and with
``--vr180``.  tests/test_jpegxf_host.py runs the same cases through the host build of the arithmetic, which tells a wrong rule from
wrong kernel plumbing."""
import ctypes as C

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import jpgdec_ref as D
import jpgxc_ref as X
import jpgxf_cases as K
import jpgxf_ref as F
from test_jpegxf_host import _with_exif, _xf_call

pytestmark = pytest.mark.gpu
CASES = K.cases()
runner = CliRunner()


class Report(C.Structure):
    _fields_ = [("segments", C.c_uint32), ("subsequences", C.c_uint32), ("rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("error_pos", C.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    from vr180_convert_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test without a visible HIP device")
    return _native.lib()


def compose(lib, datas, outputs, S=0, stream=None):
    """through the C ABI: (return code, reports, every output's file, the scans' buffer)"""
    srcs, outs, keep = _xf_call(datas, outputs)
    d0 = datas[0]
    bounds = [max(int(lib.v1c_jpeg_compose_bound(d0, len(d0), o.width, o.height, o.restart_mcus)), 1 << 12) for o in outs]
    buf = np.full(sum(bounds), 0xA5, np.uint8)
    at = 0
    for o, b in zip(outs, bounds):
        o.out_host, o.capacity = buf.ctypes.data + at, b
        at += b
    reps = (Report * len(datas))()
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = lib.v1c_jpeg_compose(0, st, len(datas), srcs, len(outputs), outs, S, reps)
    files, at = [], 0
    for o, b, spec in zip(outs, bounds, outputs):
        if rc == 0:
            si, tr = spec["regions"][0][:2]
            head = (C.c_uint8 * 2048)()
            n = lib.v1c_jpeg_header_xf(datas[si], len(datas[si]), o.width, o.height, o.restart_mcus, F.code_of(tr) >> 2,
                                       o.dht if o.optimize else None, o.dht_size, head, 2048)
            assert n > 0, lib.v1c_last_error()
            files.append(bytes(head[:n]) + buf[at:at + int(o.size)].tobytes() + b"\xff\xd9")
            assert (buf[at + int(o.size):at + b] == 0xA5).all()  # nothing behind the scan is written
        at += b
    return rc, reps, files, buf


@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_restatement(lib, name):
    datas, outputs = CASES[name]
    want = list(K.reference(name))
    rc, reps, files, _ = compose(lib, datas, outputs)
    assert rc == 0, lib.v1c_last_error()
    assert files == want, ([len(f) for f in files], [len(f) for f in want])
    assert [r.segments for r in reps] == [D.parse(d).nseg for d in datas] and all(r.rounds >= 1 and r.error_pos == 0 for r in reps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rc, reps, files, _ = compose(lib, datas, outputs, 256, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    assert rc == 0, lib.v1c_last_error()
    assert files == want and all(r.subsequences >= r.segments for r in reps)


def test_a_damaged_second_source_is_reported_in_its_own_report(lib):
    """V1C_E_CORRUPT from the device's last pass: the bit in the damaged source's report, the sound source's report clean"""
    import re

    last = None
    for name, (datas, outputs, by_parse) in K.corrupt().items():
        if by_parse:
            continue
        rc, reps, _, _ = compose(lib, datas, outputs)
        said = lib.v1c_last_error()
        assert rc == -5 and b"source 1" in said, (name, rc, said)
        assert reps[0].error_pos == 0 and reps[0].rounds >= 1 and reps[1].rounds >= 1, name
        assert reps[1].error_pos == int(re.search(rb"at bit (\d+)", said).group(1)), (name, said)
        last = (datas, outputs)
    assert last is not None
    # and the same sources in the other order: source 0 is the damaged one
    datas, outputs = last
    rc, reps, _, _ = compose(lib, datas[::-1], [dict(o, regions=[(1,) + tuple(r[1:]) for r in o["regions"]]) for o in outputs])
    assert rc == -5 and b"source 0" in lib.v1c_last_error() and reps[1].error_pos == 0


def test_coefficients_out_of_range_are_refused_after_the_gather(lib):
    for name, (datas, outputs) in K.out_of_range().items():
        rc, _, _, _ = compose(lib, datas, outputs)
        assert rc == -2 and b"coefficient" in lib.v1c_last_error(), name


def test_refused_under_stream_capture(lib):
    """the host reads flags and sizes between the kernels: under capture the call is refused before it does anything, and nothing is
    written"""
    name = "join_right_rot180_420"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    scratch = torch.zeros(16, device="cuda")
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            scratch.zero_()
            rc, reps, _, buf = compose(lib, *CASES[name], 0, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    assert rc == -2 and b"graph" in lib.v1c_last_error()
    assert (buf == 0xA5).all() and all(r.rounds == 0 for r in reps)
    rc, _, files, _ = compose(lib, *CASES[name], 0)
    assert rc == 0 and files == list(K.reference(name))


@pytest.mark.parametrize("S", [0, 256])
@pytest.mark.parametrize("name, optimize_first", [("swap_2x2_420", False), ("source_dri2_422", False), ("noise_q100_420_split", True)])
def test_one_source_untransformed_is_the_transcoder_s_call(lib, name, optimize_first, S):
    """``v1c_jpeg_transcode`` and ``v1c_jpeg_compose`` of one source with transform 0 are one host chain: the same return code, the same
    scans, sizes and tables, the same report -- over two regions, an MCU of two luma blocks with restart markers in the source, and a head
    with an optimising and an Annex K output"""
    import jpgxc_cases as XK
    from test_jpegxc_host import _xc_outputs

    data, outputs = XK.cases()[name]
    if optimize_first:
        outputs = [dict(outputs[0], optimize=True)] + list(outputs[1:])
        assert len(outputs) == 2
    st = torch.cuda.current_stream().cuda_stream

    def run(outs, call):
        bounds = [int(lib.v1c_jpeg_transcode_bound(data, len(data), o.width, o.height, o.restart_mcus)) for o in outs]
        assert all(bounds)
        buf, at = np.full(sum(bounds), 0xA5, np.uint8), 0
        for o, b in zip(outs, bounds):
            o.out_host, o.capacity = buf.ctypes.data + at, b
            at += b
        rep = Report()
        rc = call(outs, rep)
        return rc, [(int(o.size), int(o.dht_size), bytes(o.dht[:o.dht_size])) for o in outs], buf.tobytes(), (rep.segments, rep.subsequences, rep.rounds)

    xc_outs, keep_xc = _xc_outputs(outputs, X.Source(data))
    one = run(xc_outs, lambda outs, rep: lib.v1c_jpeg_transcode(0, st, data, len(data), len(outs), outs, S, C.byref(rep)))
    srcs, xf_outs, keep_xf = _xf_call([data], [dict(o, regions=[(0, 0) + tuple(r) for r in o["regions"]]) for o in outputs])
    two = run(xf_outs, lambda outs, rep: lib.v1c_jpeg_compose(0, st, 1, srcs, len(outs), outs, S, C.byref(rep)))
    assert one[0] == two[0] == 0, lib.v1c_last_error()
    assert one == two
    assert all(size > 0 for size, _, _ in one[1]) and [bool(n) for _, n, _ in one[1]] == [bool(o.get("optimize")) for o in outputs]
    assert one[3][2] >= 1 and one[3][1] >= one[3][0] >= 1


# ---- the Python entries ----------------------------------------------------------------------------------------------------------------
def _coefficients(data):
    d = D.decode(data, check=False)
    return d.info, D.dc_values(d.info, d.coef)


@pytest.mark.parametrize("kind", list(K.KINDS))
def test_transform_jpeg_equals_restatement(kind, tmp_path):
    import vr180_convert_amd as V
    from vr180_convert_amd.jpeg_compose_device import last_compose_report

    data = CASES[f"partial_trimmed_{kind}"][0][0]
    for code in K.codes_of(kind):
        op = F.NAMES[code]
        for kw in (dict(trim=True), dict(trim=True, optimize=True, restart_mcus=0)):
            assert V.transform_jpeg(data, op, **kw) == F.transform_jpeg(data, op, **kw), (op, kw)
    rep = last_compose_report()
    assert len(rep["sources"]) == 1 and rep["sources"][0]["rounds"] >= 1 and len(rep["sizes"]) == 1
    p = tmp_path / "eye.jpg"  # a path is taken as bytes are
    p.write_bytes(data)
    assert V.transform_jpeg(p, "none") == X.transcode_jpeg(data)


@pytest.mark.parametrize("kind", list(K.KINDS))
def test_join_sbs_jpeg_equals_restatement(kind):
    import vr180_convert_amd as V

    left, right = CASES[f"join_{kind}"][0]
    assert V.join_sbs_jpeg(left, right) == K.reference(f"join_{kind}")[0]
    assert V.join_sbs_jpeg(left, right, right_transform="rot180", optimize=True) == K.reference(f"join_right_rot180_{kind}")[0]
    part = CASES[f"join_trimmed_{kind}"][0][0]
    assert V.join_sbs_jpeg(part, part, left_transform="flip_v", right_transform="rot180", trim=True) == K.reference(f"join_trimmed_{kind}")[0]
    # the join of a split is the whole image, coded again
    whole = V.join_sbs_jpeg(left, right)
    assert V.join_sbs_jpeg(*V.split_sbs_jpeg(whole)) == whole


def test_sbs_from_vr180_photo_and_normalize_orientation():
    import vr180_convert_amd as V
    from vr180_convert_amd.jpeg_compose_device import EXIF_TRANSFORMS
    from vr180_convert_amd.vr180_photo import assemble_vr180_photo

    left, right = CASES["join_420"][0]
    photo = assemble_vr180_photo(left, right, 96, 32)
    assert V.sbs_from_vr180_photo(photo) == K.reference("join_420")[0]
    assert V.sbs_from_vr180_photo(photo, right_transform="rot180", optimize=True) == K.reference("join_right_rot180_420")[0]
    data = CASES["all_codes_3x2_444"][0][0]
    for order in ("II", "MM"):
        for orientation in range(1, 9):
            tagged = _with_exif(data, orientation, order)
            assert V.normalize_orientation_jpeg(tagged) == F.transform_jpeg(data, EXIF_TRANSFORMS[orientation]), (order, orientation)
    assert V.normalize_orientation_jpeg(data) == X.transcode_jpeg(data)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_cli_join_gives_back_the_file_xmp_device_split(tmp_path):
    """xmp --device, then join of the photo: a file whose coefficients are the original side-by-side file's"""
    from vr180_convert_amd import cli

    left, right = CASES["join_420"][0]
    sbs = tmp_path / "sbs.jpg"
    sbs.write_bytes(K.reference("join_420")[0])
    res = runner.invoke(cli.app, ["xmp", "--device", str(sbs)])
    assert res.exit_code == 0, (res.stdout, res.exception)
    res = runner.invoke(cli.app, ["join", str(tmp_path / "sbs.xmp.jpg")])
    assert res.exit_code == 0, (res.stdout, res.exception)
    back = (tmp_path / "sbs.xmp.sbs.jpg").read_bytes()
    s, want = _coefficients(sbs.read_bytes())
    t, got = _coefficients(back)
    assert (t.h, t.w, t.hs, t.vs) == (s.h, s.w, s.hs, s.vs) and np.array_equal(got, want)
    # two files, with a transform, to a path of the caller's
    l, r, out = tmp_path / "l.jpg", tmp_path / "r.jpg", tmp_path / "out.jpg"
    l.write_bytes(left), r.write_bytes(right)
    res = runner.invoke(cli.app, ["join", str(l), str(r), "--right-transform", "rot180", "--optimize", "--out-path", str(out)])
    assert res.exit_code == 0, (res.stdout, res.exception)
    assert out.read_bytes() == K.reference("join_right_rot180_420")[0]
    res = runner.invoke(cli.app, ["join", str(l), str(r), "--right-transform", "rot90"])
    assert res.exit_code != 0 and not (tmp_path / "l.join.jpg").exists()


def test_cli_join_vr180_round_trips_through_read_vr180_photo(tmp_path):
    from vr180_convert_amd import cli
    from vr180_convert_amd.vr180_photo import read_vr180_photo

    left, right = CASES["join_420"][0]
    l, r = tmp_path / "l.jpg", tmp_path / "r.jpg"
    l.write_bytes(left), r.write_bytes(right)
    res = runner.invoke(cli.app, ["join", str(l), str(r), "--vr180", "--right-transform", "rot180"])
    assert res.exit_code == 0, (res.stdout, res.exception)
    got_l, got_r, props = read_vr180_photo((tmp_path / "l.join.jpg").read_bytes())
    assert got_l == F.transform_jpeg(left, "none") and got_r == F.transform_jpeg(right, "rot180")
    assert dict((n, v) for _, n, v in props)["FullPanoWidthPixels"] == 96
    # the right eye turned back is the file's coefficients
    assert np.array_equal(_coefficients(F.transform_jpeg(got_r, "rot180"))[1], _coefficients(right)[1])
