"""Writer of prosper's texture cache: what Texture2D::init does when `prosper_cache/<name>.dds` is missing
or stale (src/scene/Texture.cpp:370-411) - decode the source image, compress() it, write the DDS and its tag - with the
compression on the GPU (`capi.Context.compress_texture`: mip chain, BC7 encoder).

The file is a valid cache for prosper and for `load_gltf`; its texels are this library's, not prosper's byte for byte:
the generated levels are the 2 x 2 box of DESIGN.md (f14), not stb's resize, and the BC7 blocks follow the encoder rule
of `prosper_amd.bc7.encode_blocks`, not the third-party encoder prosper links."""
import json
import os

from . import dds, structs as S
from .gltf import decode_image

_DXGI = {S.FORMAT_BC7_UNORM: dds.DXGI_FORMAT_BC7_UNORM, S.FORMAT_RGBA8_UNORM: dds.DXGI_FORMAT_R8G8B8A8_UNORM}


def build(source_path, ctx, srgb, mips=True):
    """Compresses the image file `source_path` into `prosper_cache/<name>.dds` beside it and tags it with the source's
    write time.  `ctx`: a capi.Context, or anything with its `compress_texture(rgba, srgb=, mips=)`.  `srgb`: the
    image is a base colour (Texture2DOptions::colorSpace), `mips`: Texture2DOptions::generateMipMaps.
    -> the cache file's path"""
    with open(source_path, "rb") as f:
        rgba = decode_image(f.read())
    fmt, levels = ctx.compress_texture(rgba, srgb=srgb, mips=mips)
    cached = dds.cache_path(source_path)
    os.makedirs(os.path.dirname(cached), exist_ok=True)
    dds.write_texture(cached, _DXGI[fmt], rgba.shape[1], rgba.shape[0], levels)
    dds.write_cache_tag(cached, source_path)
    return cached


def srgb_images(doc):
    """Image indices of a glTF document that prosper loads as sRGB (src/scene/DeferredLoadingContext.cpp:1130-1176): an
    image some material uses as base colour; one used only for metallic-roughness or normals is linear."""
    textures = doc.get("textures", [])
    out = set()
    for m in doc.get("materials", []):
        info = m.get("pbrMetallicRoughness", {}).get("baseColorTexture")
        if info is not None and "source" in textures[info["index"]]:
            out.add(textures[info["index"]]["source"])
    return out


def build_for_gltf(path, ctx, mips=True):
    """`build` for every image file of the .gltf at `path` whose cache is missing or stale (`dds.cache_valid`).
    A .glb keeps its images inside the file: prosper has no cache for those and nothing is written.
    -> the cache files written"""
    if path.lower().endswith(".glb"):
        return []
    with open(path, "rb") as f:
        doc = json.loads(f.read().decode("utf-8"))
    base = os.path.dirname(os.path.abspath(path))
    srgb = srgb_images(doc)
    written = []
    for index, img in enumerate(doc.get("images", [])):
        if "uri" not in img or img["uri"].startswith("data:"):
            continue
        source = os.path.join(base, img["uri"].replace("%20", " "))
        if not os.path.exists(source) or dds.cache_valid(dds.cache_path(source), source):
            continue
        written.append(build(source, ctx, index in srgb, mips))
    return written
