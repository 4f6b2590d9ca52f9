#!/usr/bin/env python3
"""Writes the two reference assets the suite reads as files, xz-compressed, from the reference's res/ directory:

    python tests/golden/make_reference_assets.py <reference>/res

  flight_helmet_gltf.tar.xz   res/glTF/FlightHelmet/glTF: FlightHelmet.gltf as it is and the images the reference's
                              checkout holds (10 of 15, .MISSING_LARGE_BLOBS lacks the rest) box-filtered to 64 x 64 (the
                              originals are 25 MB).  FlightHelmet.bin (3.4 MB) is not stored: tests/conftest.py rebuilds it
                              from tests/golden/flight_helmet.npz, and this script first checks that ingesting the shipped
                              buffer and the rebuilt one both give that fixture's geometry, byte for byte
  tony_mc_mapface.dds.xz      res/texture/tony_mc_mapface.dds, the tone-map LUT, byte for byte

Data only.  The archive is reproducible: sorted members, zero mtimes and owners."""
import io
import json
import lzma
import os
import shutil
import sys
import tarfile
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

from conftest import flight_helmet_bin  # noqa: E402
from prosper_amd import flight_helmet, gltf  # noqa: E402

TEX = 64


def small_png(path):
    img = Image.open(path)
    f = max(1, min(img.size) // TEX)
    buf = io.BytesIO()
    img.reduce(f).save(buf, format="PNG", optimize=True)
    return buf.getvalue()


def same_geometry(a, b):
    return (np.array_equal(np.concatenate(a._buffers[0]), np.concatenate(b._buffers[0])) and
            [bytes(m) for m in a.metadatas] == [bytes(m) for m in b.metadatas])


def check_rebuilt_buffer(src, doc):
    fixture = flight_helmet.load_fixture(sky_size=0)
    assert same_geometry(gltf.load_gltf(os.path.join(src, "FlightHelmet.gltf"), load_images=False), fixture)
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "FlightHelmet.gltf"), "w") as f:
        json.dump(doc, f)
    with open(os.path.join(tmp, doc["buffers"][0]["uri"]), "wb") as f:
        f.write(flight_helmet_bin(doc, fixture))
    assert same_geometry(gltf.load_gltf(os.path.join(tmp, "FlightHelmet.gltf"), load_images=False), fixture)
    shutil.rmtree(tmp)


def main(res):
    src = os.path.join(res, "glTF", "FlightHelmet", "glTF")
    path = os.path.join(src, "FlightHelmet.gltf")
    members = {"FlightHelmet.gltf": open(path, "rb").read()}
    doc = json.load(open(path))
    check_rebuilt_buffer(src, doc)
    for im in doc["images"]:
        p = os.path.join(src, im["uri"])
        if os.path.exists(p):
            members[im["uri"]] = small_png(p)
    raw = io.BytesIO()
    with tarfile.open(fileobj=raw, mode="w", format=tarfile.USTAR_FORMAT) as tar:
        for name in sorted(members):
            info = tarfile.TarInfo(name)
            info.size, info.mode = len(members[name]), 0o644
            tar.addfile(info, io.BytesIO(members[name]))
    out = os.path.join(HERE, "flight_helmet_gltf.tar.xz")
    with open(out, "wb") as f:
        f.write(lzma.compress(raw.getvalue(), preset=9 | lzma.PRESET_EXTREME))
    print("wrote %s: %.2f MB, %d files" % (out, os.path.getsize(out) / 1e6, len(members)))

    out = os.path.join(HERE, "tony_mc_mapface.dds.xz")
    with open(out, "wb") as f:
        f.write(lzma.compress(open(os.path.join(res, "texture", "tony_mc_mapface.dds"), "rb").read(), preset=9 | lzma.PRESET_EXTREME))
    print("wrote %s: %.2f MB" % (out, os.path.getsize(out) / 1e6))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
