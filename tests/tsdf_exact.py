"""The numeric contract of integration::UniformTSDFVolume (include/mi_icp.h) restated in numpy fp32: Integrate with
the depth -> camera-distance multiplier, both extractions and Raycast, vectorised over voxels and pixels (the raycast
march is a masked loop).  numpy neither fuses products nor reorders sums, and fp32 division and square root are
correctly rounded there as on the device, so every value is meant to be bit-equal to the kernels'.  A helper for
test_tsdf_cpu.py and test_gpu_tsdf.py, not a test."""
import numpy as np

F = np.float32
NO_COLOR, RGB8, GRAY32 = 0, 1, 2


class Volume:
    def __init__(self, length, resolution, sdf_trunc, color_type, origin=(0, 0, 0)):
        self.res = int(resolution)
        self.h = self.res // 2
        self.length = F(length)
        self.vl = F(F(length) / F(self.res))
        self.half = F(F(0.5) * self.vl)
        self.trunc = F(sdf_trunc)
        self.color_type = int(color_type)
        self.origin = np.asarray(origin, F).reshape(3)
        self.mult_key = None
        self.reset()

    def reset(self):
        n = self.res ** 3
        self.tsdf = np.zeros(n, F)
        self.weight = np.zeros(n, F)
        self.color = np.ones((n, 3), F)

    def grid(self, a):
        return a.reshape(self.res, self.res, self.res)


def multiplier(width, height, fx, fy, cx, cy):
    xx = (np.arange(width).astype(F) - F(cx)) * (F(1) / F(fx))
    yy = (np.arange(height).astype(F) - F(cy)) * (F(1) / F(fy))
    return np.sqrt(((xx * xx)[None, :] + (yy * yy)[:, None]) + F(1))


def integrate(vol, depth, color, width, height, fx, fy, cx, cy, extrinsic):
    """one frame into vol; depth [H, W] float32, color [H, W, 3] uint8 (RGB8) or [H, W] float32 (Gray32) or None.
    Returns the number of voxels updated."""
    fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
    E = np.asarray(extrinsic, F).reshape(4, 4)
    key = (width, height, fx, fy, cx, cy)
    if vol.mult_key != key:
        vol.mult, vol.mult_key = multiplier(width, height, fx, fy, cx, cy), key
    res, h, vl = vol.res, vol.h, vol.vl
    rel = (np.arange(res) - h).astype(F)
    px = ((vol.half + vl * rel) + vol.origin[0])[:, None, None]
    py = ((vol.half + vl * rel) + vol.origin[1])[None, :, None]
    pz = vol.half + vol.origin[2]
    zf = rel[None, None, :]
    P = []
    for r in range(3):
        base = ((E[r, 0] * px + E[r, 1] * py) + E[r, 2] * pz) + E[r, 3]
        P.append((base + zf * (vl * E[r, 2])).reshape(-1))
    idx = np.nonzero(~(P[2] <= F(0)))[0]
    X, Y, Z = P[0][idx], P[1][idx], P[2][idx]
    with np.errstate(all="ignore"):
        u_f = (X * fx / Z + cx) + F(0.5)
        v_f = (Y * fy / Z + cy) + F(0.5)
    safe_w, safe_h = F(width) - F(0.0001), F(height) - F(0.0001)
    ok = (u_f >= F(0.0001)) & (u_f < safe_w) & (v_f >= F(0.0001)) & (v_f < safe_h)
    idx, Z, u_f, v_f = idx[ok], Z[ok], u_f[ok], v_f[ok]
    u, v = np.floor(u_f).astype(np.int64), np.floor(v_f).astype(np.int64)
    d = np.asarray(depth, F)[v, u]
    ok = ~(d <= F(0))
    idx, Z, u, v, d = idx[ok], Z[ok], u[ok], v[ok], d[ok]
    sdf = (d - Z) * vol.mult[v, u]
    ok = sdf > -vol.trunc
    idx, u, v, sdf = idx[ok], u[ok], v[ok], sdf[ok]
    inv = F(1.0 / np.float64(vol.trunc))
    t = np.minimum(F(1), sdf * inv)
    w = vol.weight[idx]
    w1 = w + F(1)
    vol.tsdf[idx] = (vol.tsdf[idx] * w + t) / w1
    if vol.color_type == RGB8:
        s = np.asarray(color)[v, u].astype(F)
        vol.color[idx] = (vol.color[idx] * w[:, None] + s) / w1[:, None]
    elif vol.color_type == GRAY32:
        s = np.asarray(color, F)[v, u]
        vol.color[idx] = (vol.color[idx] * w[:, None] + s[:, None]) / w1[:, None]
    vol.weight[idx] = w1
    return int(idx.size)


def valid_mask(vol):
    return (vol.weight != F(0)) & (vol.tsdf < F(0.98)) & (vol.tsdf >= F(-0.98))


def extract_voxel_point_cloud(vol):
    """-> (points [m, 3], colors [m, 3]) in ascending voxel index"""
    res = vol.res
    idx = np.nonzero(valid_mask(vol))[0]
    x, yz = idx // (res * res), idx % (res * res)
    y, z = yz // res, yz % res
    pts = np.stack([(vol.half + vol.vl * (c - vol.h).astype(F)) + vol.origin[k] for k, c in enumerate((x, y, z))], 1)
    c = ((vol.tsdf[idx].astype(np.float64) + 1.0) * 0.5).astype(F)
    return pts.astype(F), np.stack([c, c, c], 1)


def _floor_int(x):
    """floor to int64 with the value held inside +-1e9 first, a NaN counting as -1e9"""
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(np.floor(x), F(-1.0e9)), F(1.0e9)).astype(np.int64)


def _tsdf_at(vol, p):
    """GetTSDFAt at points p [m, 3] (metres from the volume's corner)"""
    T = vol.grid(vol.tsdf)
    g = p / vol.vl - F(0.5)
    i = np.clip(_floor_int(g), 0, vol.res - 2)
    r = g - i.astype(F)
    r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
    one = F(1)
    i0, i1, i2 = i[:, 0], i[:, 1], i[:, 2]
    s = np.zeros(len(p), F)
    s = s + (one - r0) * (one - r1) * (one - r2) * T[i0, i1, i2]
    s = s + (one - r0) * (one - r1) * r2 * T[i0, i1, i2 + 1]
    s = s + (one - r0) * r1 * (one - r2) * T[i0, i1 + 1, i2]
    s = s + (one - r0) * r1 * r2 * T[i0, i1 + 1, i2 + 1]
    s = s + r0 * (one - r1) * (one - r2) * T[i0 + 1, i1, i2]
    s = s + r0 * (one - r1) * r2 * T[i0 + 1, i1, i2 + 1]
    s = s + r0 * r1 * (one - r2) * T[i0 + 1, i1 + 1, i2]
    s = s + r0 * r1 * r2 * T[i0 + 1, i1 + 1, i2 + 1]
    return s


def extract_point_cloud(vol):
    """-> (points, normals, colors or None), the candidates in ascending
    (((x-1)*(res-2) + (y-1))*(res-2) + (z-1))*3 + axis"""
    res, vl = vol.res, vol.vl
    T, V = vol.grid(vol.tsdf), vol.grid(valid_mask(vol))
    inner = slice(1, res - 1)
    m = res - 2
    cross = np.zeros((m, m, m, 3), bool)
    for ax in range(3):
        s1 = [inner] * 3
        s1[ax] = slice(2, res)
        f0, f1 = T[inner, inner, inner], T[tuple(s1)]
        c = V[inner, inner, inner] & V[tuple(s1)] & (f0 * f1 < F(0))
        last = [slice(None)] * 3
        last[ax] = m - 1          # coordinate res-2: its neighbour res-1 is not < res-1
        c[tuple(last)] = False
        cross[..., ax] = c
    x, y, z, ax = np.nonzero(cross)
    x, y, z = x + 1, y + 1, z + 1
    n = len(x)
    xyz = np.stack([x, y, z], 1)
    nb = xyz.copy()
    nb[np.arange(n), ax] += 1
    f0, f1 = T[x, y, z], T[nb[:, 0], nb[:, 1], nb[:, 2]]
    r0, r1 = np.abs(f0), np.abs(f1)
    rs = r0 + r1
    q = (vol.half + vl * xyz.astype(F)).astype(F)
    rows = np.arange(n)
    qa = q[rows, ax]
    q[rows, ax] = (qa * r1 + (qa + vl) * r0) / rs
    hres = F(vol.h) * vl
    pts = (q + vol.origin[None, :]) - hres
    cols = None
    if vol.color_type != NO_COLOR:
        C = vol.color.reshape(res, res, res, 3)
        c0, c1 = C[x, y, z], C[nb[:, 0], nb[:, 1], nb[:, 2]]
        cols = (c0 * r1[:, None] + c1 * r0[:, None]) / rs[:, None]
        if vol.color_type == RGB8:
            cols = cols / F(255)
    gap = 0.99 * np.float64(vl)
    nrm = np.zeros((n, 3), F)
    for k in range(3):
        hi, lo = q.copy(), q.copy()
        hi[:, k] = (q[:, k].astype(np.float64) + gap).astype(F)
        lo[:, k] = (q[:, k].astype(np.float64) - gap).astype(F)
        nrm[:, k] = _tsdf_at(vol, hi) - _tsdf_at(vol, lo)
    zz = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
    pos = zz > F(0)
    with np.errstate(all="ignore"):
        nrm = np.where(pos[:, None], nrm / np.sqrt(zz)[:, None], nrm)
    return pts.astype(F), nrm.astype(F), cols


def _trilinear(vol, p):
    """InterpolateTrilinearly at p [m, 3] in voxel units"""
    T = vol.grid(vol.tsdf)
    i = p.astype(np.int64)                       # p >= 0 here: truncation
    i = np.where(p < i.astype(F) + F(0.5), i - 1, i)
    d = p - (i.astype(F) + F(0.5))
    a, b, c = d[:, 0], d[:, 1], d[:, 2]
    i = np.clip(i, 0, vol.res - 2)
    i0, i1, i2 = i[:, 0], i[:, 1], i[:, 2]
    one = F(1)
    s = T[i0, i1, i2] * (one - a) * (one - b) * (one - c) + T[i0, i1, i2 + 1] * (one - a) * (one - b) * c
    s = s + T[i0, i1 + 1, i2] * (one - a) * b * (one - c)
    s = s + T[i0, i1 + 1, i2 + 1] * (one - a) * b * c
    s = s + T[i0 + 1, i1, i2] * a * (one - b) * (one - c)
    s = s + T[i0 + 1, i1, i2 + 1] * a * (one - b) * c
    s = s + T[i0 + 1, i1 + 1, i2] * a * b * (one - c)
    s = s + T[i0 + 1, i1 + 1, i2 + 1] * a * b * c
    return s


def inverse_transform(extrinsic):
    """utility::InverseTransform in fp32: (R^T, -(R^T t)), the sum left to right"""
    E = np.asarray(extrinsic, F).reshape(4, 4)
    R = E[:3, :3].T.copy()
    t = E[:3, 3]
    pt = np.array([((-R[r, 0]) * t[0] + (-R[r, 1]) * t[1]) + (-R[r, 2]) * t[2] for r in range(3)], F)
    return R, pt


def raycast(vol, width, height, fx, fy, cx, cy, extrinsic, sdf_trunc):
    """-> (points, normals, colors) [width*height, 3] in pixel order, NaN where the pixel is invalid, and the number
    of nearest-voxel tsdf gathers the march made (the first sample of every ray included)"""
    fx, fy, cx, cy, trunc = F(fx), F(fy), F(cx), F(cy), F(sdf_trunc)
    res, h, vl = vol.res, vol.h, vol.vl
    R, pt = inverse_transform(extrinsic)
    t = (pt - vol.origin).astype(F)
    n = width * height
    P = np.full((n, 3), np.nan, F)
    N = np.full((n, 3), np.nan, F)
    C = np.full((n, 3), np.nan, F)
    T = vol.grid(vol.tsdf)
    ys, xs = np.divmod(np.arange(n), width)
    with np.errstate(all="ignore"):
        pp0, pp1 = (xs.astype(F) - cx) / fx, (ys.astype(F) - cy) / fy
        d = np.stack([(R[r, 0] * pp0 + R[r, 1] * pp1) + R[r, 2] for r in range(3)], 1).astype(F)
        dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        live = dn > F(0)
        d = d / dn[:, None]
        length = F(res) * vl
        zero = F(0)
        q = [(np.where(d[:, k] > zero, zero, length) - t[k]) / d[:, k] for k in range(3)]
        tmin = np.fmax(np.fmax(q[0], q[1]), q[2])
        q = [(np.where(d[:, k] > zero, length, zero) - t[k]) / d[:, k] for k in range(3)]
        tmax = np.fmin(np.fmin(q[0], q[1]), q[2])
        ln = np.fmax(tmin, zero)
        live &= ~(ln >= tmax)
        live &= ln < F(np.inf)
        ln = ln + vl
    rays = np.nonzero(live)[0]
    d, ln = d[rays], ln[rays]

    def cell(d, at):
        with np.errstate(all="ignore"):
            return _floor_int((t[None, :] + d * at[:, None]) / vl) + h

    g = cell(d, ln)
    ok = ((g >= 0) & (g < res - 1)).all(1)
    rays, d, ln, g = rays[ok], d[ok], ln[ok], g[ok]
    cur = T[g[:, 0], g[:, 1], g[:, 2]]
    gathers = len(rays)
    mx = ln + length * F(1.41421354)
    step = trunc * F(0.5)
    ok = mx + step > mx
    rays, d, ln, cur, mx = rays[ok], d[ok], ln[ok], cur[ok], mx[ok]
    while True:
        ok = ln < mx
        rays, d, ln, cur, mx = rays[ok], d[ok], ln[ok], cur[ok], mx[ok]
        if len(rays) == 0:
            break
        g = cell(d, ln + step)
        ins = ((g >= 1) & (g < res - 1)).all(1)
        gi = np.where(ins[:, None], g, 0)
        new = T[gi[:, 0], gi[:, 1], gi[:, 2]]
        gathers += int(ins.sum())
        prev = cur
        cur = np.where(ins, new, cur)
        out_in = ins & (prev < zero) & (cur > zero)           # left the surface from behind: invalid
        hit = ins & (prev > zero) & (cur < zero)
        if hit.any():
            hr, hd, hl, hp, hc = rays[hit], d[hit], ln[hit], prev[hit], cur[hit]
            ts = hl - step * hp / (hc - hp)
            vtx = t[None, :] + hd * ts[:, None]
            loc = vtx / vl + F(h)
            top = F(res - 1)
            one = F(1)
            good = ((loc >= one) & (loc < top)).all(1)
            good &= ((loc + one < top) & (loc - one >= one)).all(1)
            hr, vtx, loc = hr[good], vtx[good], loc[good]
            nr = np.zeros((len(hr), 3), F)
            for k in range(3):
                e = np.zeros(3, F)
                e[k] = one
                nr[:, k] = _trilinear(vol, loc + e[None, :]) - _trilinear(vol, loc - e[None, :])
            nn = np.sqrt((nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2])
            good = ~(nn == zero)
            hr, vtx, loc, nr, nn = hr[good], vtx[good], loc[good], nr[good], nn[good]
            with np.errstate(all="ignore"):
                N[hr] = nr / nn[:, None]
            P[hr] = vtx + vol.origin[None, :]
            li = loc.astype(np.int64)
            ci = (li[:, 0] * res + li[:, 1]) * res + li[:, 2]
            if vol.color_type == RGB8:
                C[hr] = (vol.color[ci].astype(np.float64) / 255.0).astype(F)
            elif vol.color_type == GRAY32:
                C[hr] = vol.color[ci]
            else:
                C[hr] = zero
        go = ~(out_in | hit)
        rays, d, ln, cur, mx = rays[go], d[go], ln[go], cur[go], mx[go]
        ln = ln + step
    return P, N, C, gathers


# ---- inputs shared by the tests -------------------------------------------------------------------------------------
PRIMESENSE = (640, 480, 525.0, 525.0, 319.5, 239.5)       # PinholeCameraIntrinsicParameters::PrimeSenseDefault


def load_rgbd_frames(root):
    """the reference's five RGB-D frames (tests/golden/rgbd): [(depth float32 [480, 640] in metres with values >= 4
    set to 0, colour uint8 [480, 640, 3], extrinsic = inverse of the frame's pose)], as the reference's RealData test
    prepares them (RGBDImage::CreateFromColorAndDepth(color, depth, 1000, 4, false): the depth rule of include/mi_icp.h
    "image", value * the correctly rounded reciprocal of the scale, pinned by the reference's own vector)"""
    import os
    from PIL import Image
    lines = open(os.path.join(root, "odometry.log")).read().split("\n")
    frames = []
    k = 0
    while k * 5 + 4 < len(lines) and lines[k * 5].strip():
        pose = np.array([[float(x) for x in lines[k * 5 + 1 + r].split()] for r in range(4)], F)
        d = np.asarray(Image.open(os.path.join(root, "depth", "%05d.png" % k))).astype(F) * F(np.float64(1.0) / np.float64(F(1000)))
        d = np.where(d >= F(4.0), F(0), d).astype(F)
        c = np.ascontiguousarray(np.asarray(Image.open(os.path.join(root, "color", "%05d.jpg" % k)).convert("RGB")))
        frames.append((d, c, np.linalg.inv(pose).astype(F)))
        k += 1
    return frames


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """extrinsic (world -> camera, camera looks along +z) of a camera at `eye` looking at `target`"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                     # rows: camera axes in world coordinates
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ eye
    return E.astype(F)


def render_scene(width, height, fx, fy, cx, cy, extrinsic, planes, sphere=None, holes=True):
    """depth (float32, the camera-frame z) and colour (uint8 x 3) images of planes [(normal, offset): n.p = offset]
    and a sphere (centre, radius) in world coordinates; every 11th pixel of a diagonal pattern, and everything the
    rays miss, has depth 0"""
    E = np.asarray(extrinsic, np.float64)
    R, t = E[:3, :3].T, -E[:3, :3].T @ E[:3, 3]
    ys, xs = np.mgrid[0:height, 0:width]
    dirs = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs, np.float64)], -1) @ R.T
    best = np.full((height, width), np.inf)
    with np.errstate(all="ignore"):
        for nrm, off in planes:
            nrm = np.asarray(nrm, np.float64)
            s = (off - nrm @ t) / (dirs @ nrm)
            best = np.where((s > 1e-6) & (s < best), s, best)
        if sphere is not None:
            c, rad = np.asarray(sphere[0], np.float64), float(sphere[1])
            oc = t - c
            a, b, cc = (dirs * dirs).sum(-1), 2.0 * (dirs @ oc), oc @ oc - rad * rad
            disc = b * b - 4 * a * cc
            s = (-b - np.sqrt(disc)) / (2 * a)
            best = np.where((disc > 0) & (s > 1e-6) & (s < best), s, best)
    depth = np.where(np.isfinite(best), best, 0.0)
    if holes:
        depth[(xs * 7 + ys * 13) % 11 == 0] = 0.0
    color = np.stack([(xs * 3 + ys) % 256, (xs + ys * 5) % 256, (xs * ys) % 256], -1).astype(np.uint8)
    return depth.astype(F), np.ascontiguousarray(color)
