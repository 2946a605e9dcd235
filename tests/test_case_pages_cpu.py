"""utils/case_pages.py without a GPU: the PNG writer read back chunk by chunk, the palette's control points, the case
selection, and the page builder fed synthetic scanlines."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

from cae_tools_amd.utils import case_pages


def parse_png(data):
    """[(chunk type, chunk data)] of a PNG, every CRC checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    (at, chunks) = (8, [])
    while at < len(data):
        (length,) = struct.unpack_from(">I", data, at)
        kind = data[at + 4:at + 8]
        body = data[at + 8:at + 8 + length]
        (crc,) = struct.unpack_from(">I", data, at + 8 + length)
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        at += 12 + length
    assert at == len(data)
    return chunks


def decode_png(data):
    """(width, height, scanline bytes, palette bytes, tRNS bytes) of an 8-bit palette PNG"""
    chunks = parse_png(data)
    assert [k for (k, _) in chunks] == [b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"]
    (width, height, depth, colour, compression, flt, interlace) = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, flt, interlace) == (8, 3, 0, 0, 0)
    return width, height, zlib.decompress(chunks[3][1]), chunks[1][1], chunks[2][1]


def _scanlines(rng, height, width):
    rows = rng.integers(0, 256, size=(height, width + 1), dtype=np.uint8)
    rows[:, 0] = 0
    return rows


@pytest.mark.parametrize("height,width", [(1, 1), (3, 5), (64, 63)])
def test_png_round_trip(height, width):
    rows = _scanlines(np.random.default_rng(height * 100 + width), height, width)
    (w, h, raw, plte, trns) = decode_png(case_pages.png_palette(rows, width, height))
    assert (w, h) == (width, height)
    assert raw == rows.tobytes()
    assert len(plte) == 3 * 256 and trns[:1] == b"\x00" and len(trns) <= 256


def test_png_refuses_a_wrong_length():
    with pytest.raises(ValueError):
        case_pages.png_palette(bytes(10), 3, 3)


def test_palette():
    pal = case_pages.palette()
    assert len(pal) == 256
    assert pal[0][3] == 0 and all(entry[3] == 255 for entry in pal[1:])
    assert pal[1][:3] == (59, 76, 192) and pal[128][:3] == (221, 221, 221) and pal[255][:3] == (180, 4, 38)
    # linear in between, rounded half up
    for (j, (a, b)) in ((40, ((59, 76, 192), (221, 221, 221))), (127 + 63, ((221, 221, 221), (180, 4, 38)))):
        s = (j if j <= 127 else j - 127) / 127.0
        assert pal[1 + j][:3] == tuple(int(np.floor(ca + (cb - ca) * s + 0.5)) for (ca, cb) in zip(a, b))
    # the PLTE chunk of a written file is this table
    (_, _, _, plte, _) = decode_png(case_pages.colour_bar())
    assert plte == bytes(c for entry in pal for c in entry[:3])
    (w, h, raw, _, _) = decode_png(case_pages.colour_bar())
    assert (w, h) == (255, 1) and raw == bytes([0]) + bytes(range(1, 256))


@pytest.mark.parametrize("n,k", [(10, None), (10, 3), (3, 10), (0, 5)])
def test_select_cases(n, k):
    got = case_pages.select_cases(n, k)
    assert len(got) == (n if k is None else min(k, n))
    assert got == sorted(set(got))
    assert all(0 <= i < n for i in got)
    if k is not None and n:
        assert got == [i * n // min(k, n) for i in range(min(k, n))]


def test_page_builder(tmp_path):
    rng = np.random.default_rng(3)
    cases = [0, 4, 8, 12, 16]
    mse = np.array([0.5, 2.0, 0.5, np.nan, 0.25])
    mae = np.sqrt(np.nan_to_num(mse))
    names = ["lowres", "hires", "model_output", "error"]
    shapes = {"lowres": (3, 5), "hires": (8, 7), "model_output": (8, 7), "error": (8, 7)}
    layers = []
    for (k, name) in enumerate(names):
        (h, w) = shapes[name]
        layers.append((name, -1.0 - k, 2.0 + k, np.stack([_scanlines(rng, h, w) for _ in cases])))
    folder = str(tmp_path / "test")
    path = case_pages.write_case_pages(folder, "test", cases, layers, {"mae": mae, "mse": mse},
                                       times=np.array([10.0, 11.0, 12.0, 13.0, 14.0]), time_units="days since 2000-01-01")
    assert path == os.path.join(folder, "index.html")
    with open(path) as f:
        page = f.read()
    # rows by descending mse (NaN first, as the worst), ties by case index
    assert [int(c) for c in re.findall(r'<tr class="case" data-case="(\d+)"', page)] == [12, 4, 0, 8, 16]
    # the layers in the order given, each with its range
    assert re.findall(r'data-layer="([^"]+)"', page) == names
    assert "-1 … 2" in page and "-4 … 5" in page
    assert "days since 2000-01-01" in page and "image-rendering: pixelated" in page
    # every image the page names exists and decodes to the scanlines of its case and layer
    srcs = re.findall(r'<img[^>]* src="([^"]+)"', page)
    assert len(srcs) == len(names) + len(cases) * len(names)
    for src in srcs:
        assert os.path.isfile(os.path.join(folder, src)), src
    rows = page.split('<tr class="case"')[1:]
    for (row, case) in zip(rows, [12, 4, 0, 8, 16]):
        assert re.findall(r'src="images/(case\d+_[^"]+\.png)"', row) == [f"case{case:06d}_{n}.png" for n in names]
        assert 'width="250"' in row
        for (name, _, _, scan) in layers:
            with open(os.path.join(folder, "images", f"case{case:06d}_{name}.png"), "rb") as f:
                (w, h, raw, _, _) = decode_png(f.read())
            assert (h, w + 1) == scan.shape[1:] and raw == scan[cases.index(case)].tobytes()
