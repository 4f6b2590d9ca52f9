"""A deterministic meshlet builder of our own, in prosper's layout.

prosper partitions a mesh with meshoptimizer (generateMeshlets, src/scene/DeferredLoadingContext.cpp:378-440); the
partition itself is no contract, the LAYOUT is, and that is what this module writes:

  meshlets          4 u32 each: vertexOffset, triangleOffset, vertexCount, triangleCount (meshopt_Meshlet); at most
                    MAX_VERTICES vertices and MAX_TRIANGLES triangles (Utils.hpp sMaxMsVertices / sMaxMsTriangles)
  meshletBounds     5 u32 each: centre xyz and radius (float32), then coneAxisS8.xyz | coneCutoffS8 << 24
  meshletVertices   indices into the mesh's vertices, u32 here; u16 in the buffer when the mesh usesShortIndices
  meshletTriangles  u8 triplets of indices into the meshlet's vertices; every meshlet starts on a 4-byte boundary as
                    meshoptimizer's do, and the array is padded as generateMeshlets pads it

The partition is a greedy scan of the index buffer in order: a triangle goes into the current meshlet unless it would
take it past either limit.  The bounds are conservative on purpose:

  sphere  centre = the middle of the vertices' box (float32); radius = the largest distance of a vertex from that
          float32 centre, taken in float64 and rounded UP to float32: every vertex lies inside.
  cone    what meshopt_computeMeshletBounds documents, for the test draw_list_culler.comp makes:
              dot(centre - eye, axis) >= cutoff * |centre - eye| + radius   =>   every triangle is back-facing.
          axis = the normalised sum of the triangles' unit normals, quantised to s8 FIRST; the cutoff is then taken
          against the axis the shader will see (the decoded one, normalised): sin of the largest angle between it and
          a normal, in float64, rounded up to the next s8 step and one more.  Where the normals span a hemisphere or
          close to it (smallest cosine <= 0.1, meshoptimizer's threshold) the cone is (0, 0, 0), 127: never hidden.
"""
import numpy as np

MAX_VERTICES = 64    # sMaxMsVertices
MAX_TRIANGLES = 124  # sMaxMsTriangles


def _round_up_f32(x):
    """the smallest float32 that is not below the float64 x"""
    f = np.float32(x)
    return f if float(f) >= x else np.nextafter(f, np.float32(np.inf))


def _s8(v):
    return np.clip(np.rint(np.asarray(v, np.float64) * 127.0), -127, 127).astype(np.int32)


def decode_cone(word):
    """bounds word 4 -> (axis as the s8 triple / 127 in float64, cutoff / 127)"""
    b = np.array([word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF, (word >> 24) & 0xFF], np.uint8).view(np.int8)
    return b[:3].astype(np.float64) / 127.0, float(b[3]) / 127.0


def meshlet_bounds(points, triangles, ordered=False):
    """`points` [n, 3] of the meshlet's vertices, `triangles` [m, 3] into them -> the five bounds words.  `ordered`: the
    cone's dot products are elementwise float64 products added as (x*sx + y*sy) + z*sz, an order a kernel can follow
    (csrc/pt_mesh_prepare.hip does); the default leaves them to the matrix product."""
    p = np.asarray(points, np.float64)
    centre = ((p.min(axis=0) + p.max(axis=0)) * 0.5).astype(np.float32)
    radius = _round_up_f32(float(np.sqrt(((p - centre.astype(np.float64)) ** 2).sum(axis=1)).max()))
    t = p[np.asarray(triangles, np.int64)]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    length = np.sqrt((n * n).sum(axis=1))
    n = n[length > 0] / length[length > 0, None]  # (a degenerate triangle faces nowhere)
    axis_s8, cutoff_s8 = np.zeros(3, np.int32), 127
    if len(n):
        s = n.sum(axis=0)
        if np.sqrt((s * s).sum()) > 0:
            q = _s8(s / np.sqrt((s * s).sum()))
            seen = q.astype(np.float64)
            if (seen * seen).sum() > 0:
                seen /= np.sqrt((seen * seen).sum())
                if ordered:
                    mindp = float(((n[:, 0] * seen[0] + n[:, 1] * seen[1]) + n[:, 2] * seen[2]).min())
                else:
                    mindp = float((n @ seen).min())
                if mindp > 0.1:
                    c = int(np.ceil(np.sqrt(max(0.0, 1.0 - mindp * mindp)) * 127.0)) + 1
                    if c < 127:
                        axis_s8, cutoff_s8 = q, c
    cone = (int(axis_s8[0]) & 0xFF) | ((int(axis_s8[1]) & 0xFF) << 8) | ((int(axis_s8[2]) & 0xFF) << 16) | ((cutoff_s8 & 0xFF) << 24)
    words = np.empty(5, np.uint32)
    words[:3] = centre.view(np.uint32)
    words[3] = np.float32(radius).view(np.uint32)
    words[4] = cone
    return words


def build_meshlets(positions, indices, ordered=False):
    """-> dict(meshlets uint32 [n, 4], bounds uint32 [n, 5], vertices uint32 [k], triangles uint8 [padded]);
    `ordered` as in meshlet_bounds"""
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    indices = np.asarray(indices, np.int64).reshape(-1, 3)
    meshlets, vertices, triangles = [], [], bytearray()
    local, tri_offset, count = {}, 0, 0

    def close():
        nonlocal local, tri_offset, count
        if count:
            meshlets.append((len(vertices) - len(local), tri_offset, len(local), count))
            tri_offset = (tri_offset + 3 * count + 3) & ~3  # meshoptimizer keeps every meshlet's triangles 4-byte aligned
            triangles.extend(b"\0" * (tri_offset - len(triangles)))
        local, count = {}, 0

    for tri in indices.tolist():
        new = len({v for v in tri if v not in local})
        if len(local) + new > MAX_VERTICES or count + 1 > MAX_TRIANGLES:
            close()
        for v in tri:
            if v not in local:
                local[v] = len(local)
                vertices.append(v)
            triangles.append(local[v])
        count += 1
    close()
    m = np.array(meshlets, np.uint32).reshape(-1, 4)
    v = np.array(vertices, np.uint32)
    size = 0
    if len(m):
        # generateMeshlets: aligned_offset(last.triangle_offset + last.triangle_count, 4) * 3 bytes
        size = ((int(m[-1, 1]) + int(m[-1, 3]) + 3) & ~3) * 3
    t = np.zeros(max(size, len(triangles)), np.uint8)
    t[:len(triangles)] = np.frombuffer(bytes(triangles), np.uint8)
    assert t.size % 4 == 0
    bounds = np.empty((len(m), 5), np.uint32)
    for i, (vo, to, vc, tc) in enumerate(m.tolist()):
        bounds[i] = meshlet_bounds(positions[v[vo:vo + vc]], t[to:to + 3 * tc].reshape(-1, 3), ordered=ordered)
    return dict(meshlets=m, bounds=bounds, vertices=v, triangles=t)


def pack_sections(built, short):
    """The four sections as u32 words in writeCache's order -> [(name, words)]: meshlets, meshletBounds, meshletVertices
    (u16, padded to four bytes, when `short`), meshletTriangles."""
    v = built["vertices"]
    if short:
        v16 = v.astype(np.uint16)
        if v16.size % 2:
            v16 = np.concatenate([v16, np.zeros(1, np.uint16)])
        vwords = v16.view(np.uint32)
    else:
        vwords = v.astype(np.uint32)
    return [("meshlets", built["meshlets"].reshape(-1).astype(np.uint32)), ("bounds", built["bounds"].reshape(-1).astype(np.uint32)),
            ("vertices", vwords), ("triangles", np.ascontiguousarray(built["triangles"]).view(np.uint32))]


def read_meshlets(buffer_words, metadata, mesh_info):
    """The meshlets of a mesh back out of its geometry buffer through its GeometryMetadata, as the shaders read them
    -> the dict build_meshlets gives (triangles: the bytes up to the last meshlet's end)."""
    words = np.ascontiguousarray(buffer_words, np.uint32)
    n = mesh_info.meshletCount
    m = words[metadata.meshletsOffset:metadata.meshletsOffset + 4 * n].reshape(n, 4).copy()
    b = words[metadata.meshletBoundsOffset:metadata.meshletBoundsOffset + 5 * n].reshape(n, 5).copy()
    vcount = int(m[-1, 0] + m[-1, 2]) if n else 0
    if metadata.usesShortIndices == 1:
        v = words.view(np.uint16)[metadata.meshletVerticesOffset:metadata.meshletVerticesOffset + vcount].astype(np.uint32)
    else:
        v = words[metadata.meshletVerticesOffset:metadata.meshletVerticesOffset + vcount].copy()
    tbytes = int(m[-1, 1] + 3 * m[-1, 3]) if n else 0
    t = words.view(np.uint8)[metadata.meshletTrianglesByteOffset:metadata.meshletTrianglesByteOffset + tbytes].copy()
    return dict(meshlets=m, bounds=b, vertices=v, triangles=t)
