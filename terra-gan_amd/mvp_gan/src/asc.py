"""The ESRI ASCII grid files of the raster tools: rasters, masks and integer grids in and out, and the opening lines every
tool's main() shares (pure numpy; no torch, no GPU)."""
import numpy as np

_ASC_KEYS = ("ncols", "nrows", "xllcorner", "xllcenter", "yllcorner", "yllcenter", "cellsize", "nodata_value")


def read_asc(path):
    """-> (float32 array [nrows][ncols], header): header is a list of (key, value string) in file order, kept verbatim
    so that write_asc reproduces it."""
    header = []
    with open(path) as f:
        lines = f.readlines()
    i = 0
    while i < len(lines):
        tok = lines[i].split()
        if len(tok) == 2 and tok[0].lower() in _ASC_KEYS:
            header.append((tok[0], tok[1]))
            i += 1
        else:
            break
    keys = {k.lower() for k, _ in header}
    if not {"ncols", "nrows", "cellsize"} <= keys or not (keys & {"xllcorner", "xllcenter"}) or \
            not (keys & {"yllcorner", "yllcenter"}):
        raise ValueError(f"{path}: not an ESRI ASCII grid (header {header})")
    nrows, ncols = int(asc_value(header, "nrows")), int(asc_value(header, "ncols"))
    vals = np.array(" ".join(lines[i:]).split(), dtype=np.float32)
    if vals.size != nrows * ncols:
        raise ValueError(f"{path}: {vals.size} values for a {nrows}x{ncols} grid")
    return vals.reshape(nrows, ncols), header


def asc_value(header, key, default=None):
    for k, v in header:
        if k.lower() == key.lower():
            return v
    return default


def asc_nodata(header):
    v = asc_value(header, "NODATA_value")
    return None if v is None else float(v)


def with_nodata(header):
    """The header itself when it has a NODATA_value, else a copy with NODATA_value -9999 appended: for a raster that may
    hold NaN."""
    return header if asc_value(header, "NODATA_value") is not None else header + [("NODATA_value", "-9999")]


def write_asc(path, arr, header):
    """Write [nrows][ncols] values under `header` (as read_asc returns it).  float32 values are written with 9
    significant digits (they read back bit for bit); NaN is written as the header's NODATA_value when it has one."""
    arr = np.asarray(arr, dtype=np.float32)
    nrows, ncols = int(asc_value(header, "nrows")), int(asc_value(header, "ncols"))
    if arr.shape != (nrows, ncols):
        raise ValueError(f"write_asc: array {arr.shape} does not match the header's {nrows}x{ncols}")
    nd = asc_value(header, "NODATA_value")
    with open(path, "w") as f:
        for k, v in header:
            f.write(f"{k} {v}\n")
        for row in arr:
            txt = ["%.9g" % v for v in row.tolist()]
            if nd is not None:
                txt = [nd if t == "nan" else t for t in txt]
            f.write(" ".join(txt) + "\n")


def write_int_asc(path, arr, header):
    """An integer grid under read_asc's header, without its NODATA_value (every code is a value); exact for any int32."""
    arr = np.asarray(arr)
    if arr.shape != (int(asc_value(header, "nrows")), int(asc_value(header, "ncols"))):
        raise ValueError(f"write_int_asc: array {arr.shape} does not match the header")
    with open(path, "w") as f:
        for k, v in header:
            if k.lower() != "nodata_value":
                f.write(f"{k} {v}\n")
        for row in arr.astype(np.int64):
            f.write(" ".join(map(str, row.tolist())) + "\n")


def read_mask(path, shape):
    if path.lower().endswith(".asc"):
        mk, _ = read_asc(path)
    else:
        from PIL import Image
        mk = np.asarray(Image.open(path).convert("L"))
    if mk.shape != shape:
        raise ValueError(f"mask {path} is {mk.shape[0]}x{mk.shape[1]}, the raster {shape[0]}x{shape[1]} (no resizing)")
    return mk != 0


def write_mask(path, m, header):
    """A 0 / 1 map as .asc (under the raster's header, without its NODATA_value) or as an 8-bit image (255 = 1)."""
    m = np.asarray(m)
    if str(path).lower().endswith(".asc"):
        write_asc(path, (m != 0).astype(np.float32), [(k, v) for k, v in header if k.lower() != "nodata_value"])
    else:
        from PIL import Image
        Image.fromarray(((m != 0) * 255).astype(np.uint8)).save(path)


def read_inputs(a):
    """The opening of a tool's main(): a is its argparse namespace with dem, optionally mask and nodata (no nodata attribute,
    or None: the header's NODATA_value) -> (dem float32 [nrows][ncols], header, mask bool or None, nodata, cellsize)."""
    dem, header = read_asc(a.dem)
    mask = read_mask(a.mask, dem.shape) if getattr(a, "mask", None) else None
    nodata = getattr(a, "nodata", None)
    if nodata is None:
        nodata = asc_nodata(header)
    return dem, header, mask, nodata, float(asc_value(header, "cellsize"))
