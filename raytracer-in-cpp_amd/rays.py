"""Host ray generators for the device ray queries (Context.closest_hits, Context.trace_rays_device): float32 numpy, (origins, dirs) of
shape (height * width, 3), row-major (ray j * width + i belongs to pixel column i, row j).  They show that a camera other than the
pinhole frame is a few lines away; they are not a frame path of their own."""
import numpy as np


def orthographic_rays(cam, width, height, half_height):
    """Parallel rays through the raster points of `cam`'s screen plane (the plane at view depth 1 that the pinhole frame aims at).

    Order of operations, every step rounded to float32 unless it says double (m = cam.inv_view as 3 x 4, row-major):
      n0 = float32(2.0 * i / width - 1.0), n1 = float32(1.0 - 2.0 * j / height)     (double, then one rounding: the raster point (i, j))
      sx = float32(width) / float32(height) * float32(half_height);  x = n0 * sx;  y = n1 * float32(half_height)
      origin[r] = ((m[r][0] * x + m[r][1] * y) + m[r][2] * -1.0) + m[r][3]
      dir[r]    = -m[r][2]                                                          (the view axis: the same three floats for every ray)
    So the window is 2 * half_height world units high and width / height times as wide, row 0 at the top."""
    f = np.float32
    m = np.asarray(list(cam.inv_view), f).reshape(3, 4)
    i = np.arange(int(width), dtype=np.float64)
    j = np.arange(int(height), dtype=np.float64)
    n0 = (2.0 * i / float(width) - 1.0).astype(f)
    n1 = (1.0 - 2.0 * j / float(height)).astype(f)
    sx = f(f(width) / f(height)) * f(half_height)
    x = np.broadcast_to((n0 * sx)[None, :], (int(height), int(width)))
    y = np.broadcast_to((n1 * f(half_height))[:, None], (int(height), int(width)))
    origins = np.empty((int(height), int(width), 3), f)
    for r in range(3):
        origins[..., r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * f(-1.0)) + m[r, 3]
    dirs = np.empty_like(origins)
    dirs[...] = -m[:, 2]
    return origins.reshape(-1, 3), dirs.reshape(-1, 3)


def panorama_rays(center, width, height):
    """Equirectangular rays from the point `center`: the full sphere, pixel centres, unit directions.

    Order of operations, in double until the last step:
      lon = 2 pi (i + 0.5) / width - pi,  lat = pi (j + 0.5) / height           (column -> longitude, row -> polar angle from +y)
      d = (sin(lat) sin(lon), cos(lat), -sin(lat) cos(lon));  d = d / |d|;  dir = float32(d)
      origin = float32(center) for every ray
    So row 0 looks up (+y), the middle column looks along -z (the default camera's view axis), longitude grows towards +x."""
    i = np.arange(int(width), dtype=np.float64)
    j = np.arange(int(height), dtype=np.float64)
    lon = (2.0 * np.pi * (i + 0.5) / float(width) - np.pi)[None, :]
    lat = (np.pi * (j + 0.5) / float(height))[:, None]
    d = np.stack([np.sin(lat) * np.sin(lon), np.cos(lat) * np.ones_like(lon), -np.sin(lat) * np.cos(lon)], axis=-1)
    d /= np.sqrt((d * d).sum(axis=-1, keepdims=True))
    dirs = d.astype(np.float32).reshape(-1, 3)
    origins = np.broadcast_to(np.asarray(center, np.float32).reshape(1, 3), dirs.shape).copy()
    return origins, dirs
