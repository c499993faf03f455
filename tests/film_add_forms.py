"""Film::AddSample restated in float32 numpy, for the tests of rt_film_add_device: Scene::Render's radiance check (core/scene.cpp:60-74) and
ImageFilm::AddSample (film/image.cpp:103-142) applied sample by sample in index order.  Every product and every sum is a float32 operation of
its own (the reference is built without contraction); Ceil2Int / Floor2Int and the min(..., FILTER_TABLE_SIZE - 1) index are as written there.
A helper, no test: tests/test_film_add_host.py pins it to the frozen CPU oracle, tests/test_gpu_film_add.py to the device's films."""
import numpy as np

F = np.float32
FILTER_TABLE_SIZE = 16
Y_WEIGHT = (F(0.212671), F(0.715160), F(0.072169))          # Spectrum::YWeight, color.cpp:35-43


def checked_radiance(rgb):
    """scene.cpp:60-74 for rgb [N, 3]: (the radiances with the bad ones set to 0, which ones were bad).  Spectrum::y() (color.h:185-190) sums
    YWeight[i] * c[i] from 0 in float; `Ls.y() < -1e-5` compares the float with a double."""
    rgb = np.ascontiguousarray(rgb, F)
    with np.errstate(all="ignore"):
        y = np.zeros(len(rgb), F)
        for i in range(3):
            y = y + Y_WEIGHT[i] * rgb[:, i]
        bad = np.isnan(rgb).any(1) | (y.astype(np.float64) < -1e-5) | np.isinf(y)
    out = rgb.copy()
    out[bad] = 0
    return out, bad


def film_geometry(rd):
    """what AddSample reads of a frame, from ParsedScene.render_struct()"""
    return dict(x_pixel_start=int(rd.x_pixel_start), y_pixel_start=int(rd.y_pixel_start), x_pixel_count=int(rd.x_pixel_count), y_pixel_count=int(rd.y_pixel_count),
                x_width=F(rd.filter_x_width), y_width=F(rd.filter_y_width), table=np.array(list(rd.filter_table), F))


def add_samples(records, geom, accum=None):
    """records [N, 6] = L.r, L.g, L.b, alpha, imageX, imageY, added in index order on top of accum [5, H, W] (zeros when None).  Returns
    (accum [5, H, W] float32, the number of bad samples)."""
    rec = np.ascontiguousarray(records, F)
    xps, yps, w, h = geom["x_pixel_start"], geom["y_pixel_start"], geom["x_pixel_count"], geom["y_pixel_count"]
    xw, yw, table = F(geom["x_width"]), F(geom["y_width"]), np.ascontiguousarray(geom["table"], F)
    inv_x, inv_y = F(1) / xw, F(1) / yw
    acc = np.zeros((5, h, w), F) if accum is None else np.array(accum, F, copy=True)
    assert acc.shape == (5, h, w)
    L, bad = checked_radiance(rec[:, :3])
    alpha = rec[:, 3]
    with np.errstate(all="ignore"):
        dx, dy = rec[:, 4] - F(0.5), rec[:, 5] - F(0.5)
        x0 = np.maximum(np.ceil(dx - xw).astype(np.int64), xps); x1 = np.minimum(np.floor(dx + xw).astype(np.int64), xps + w - 1)
        y0 = np.maximum(np.ceil(dy - yw).astype(np.int64), yps); y1 = np.minimum(np.floor(dy + yw).astype(np.int64), yps + h - 1)
        for i in np.nonzero((x1 - x0 >= 0) & (y1 - y0 >= 0))[0]:
            xs = np.arange(x0[i], x1[i] + 1).astype(F); ys = np.arange(y0[i], y1[i] + 1).astype(F)
            fx = np.abs((xs - dx[i]) * inv_x * F(FILTER_TABLE_SIZE)); fy = np.abs((ys - dy[i]) * inv_y * F(FILTER_TABLE_SIZE))
            ifx = np.minimum(np.floor(fx).astype(np.int64), FILTER_TABLE_SIZE - 1); ify = np.minimum(np.floor(fy).astype(np.int64), FILTER_TABLE_SIZE - 1)
            wt = table[ify[:, None] * FILTER_TABLE_SIZE + ifx[None, :]]
            win = (slice(y0[i] - yps, y1[i] + 1 - yps), slice(x0[i] - xps, x1[i] + 1 - xps))
            for c in range(3):
                acc[c][win] += wt * L[i, c]                   # Spectrum::AddWeighted, color.h:116-120
            acc[3][win] += alpha[i] * wt
            acc[4][win] += wt
    return acc, int(bad.sum())


def unjittered_positions(rd):
    """imageX, imageY [N, 2] of an unjittered stratified frame in the sampler's order (pixel * spp + s): StratifiedSample2D's (x + .5f) * dx with
    dx = 1.f / nx (sampling.cpp:72-83) shifted by the pixel (stratified.cpp:99-117), then the ++ / -- of scene.cpp:47-53 in float"""
    xs, ys = int(rd.x_samples), int(rd.y_samples)
    px, py = np.meshgrid(np.arange(rd.x_start, rd.x_end), np.arange(rd.y_start, rd.y_end))
    sy, sx = np.divmod(np.arange(xs * ys), xs)
    ix = ((sx.astype(F) + F(0.5)) * (F(1) / F(xs)))[None, :] + px.reshape(-1, 1).astype(F)
    iy = ((sy.astype(F) + F(0.5)) * (F(1) / F(ys)))[None, :] + py.reshape(-1, 1).astype(F)
    xy = np.stack([ix.reshape(-1), iy.reshape(-1)], 1).astype(F)
    return (xy + F(1)) - F(1)
