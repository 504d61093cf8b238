"""Make the reference package use this implementation without editing it.

``install()`` rebinds the three names the reference's orchestrator and SOG writer resolve
at call time:
    gsconverter.converter.DataProcessor            (converter.py:10 -> used at :150; bound to ChainedDataProcessor,
                                                    which keeps the coordinates in HBM across density -> SOR and whose
                                                    filter methods return None -- the orchestrator ignores them)
    gsconverter.processing.DataProcessor / gsconverter.processing.data_processor.DataProcessor
                                                   (the EAGER class: every method returns self.data like the reference)
    gsconverter.formats.sog.gpu_ops                (sog.py:11 -> used at :402,443,524,544)
    gsconverter.processing.gpu_ops                 (data_processor.py:142 imports it lazily)
so ``gsconverter``'s CLI (main.py) and every flag in SURVEY.md 8(b) keep working.
"""
from __future__ import annotations

import importlib
import sys

_saved = {}


def install(sog_writer: bool = True, spz_writer: bool = True, ksplat_writer: bool = True, splat_writer: bool = True,
            cply_reader: bool = True, ksplat_reader: bool = True, spz_reader: bool = True, sog_reader: bool = True,
            splat_reader: bool = False, ply_reader: bool = True, ply_writer: bool = True, parquet_reader: bool = False,
            parquet_writer: bool = False):
    """sog_writer: also rebind ``gsconverter.formats.sog.SogFormat.write`` to formats/sog_writer.py:write_sog (spatial
    sort, quaternion packing, codebook quantiser and SH palette on the GPU; identical bytes where the reference is
    deterministic) and ``gsconverter.formats.compressed_ply.CompressedPlyFormat.write`` to
    formats/compressed_ply_writer.py:write_compressed_ply (Morton order, chunk bounds and packers on the GPU).
    spz_writer: also rebind ``gsconverter.formats.spz.SpzFormat.write`` to formats/spz_writer.py:write_spz (SH-degree scan and
    the whole body on the GPU; identical file bytes).  A reference without that module is left as it is.
    ksplat_writer: also rebind ``gsconverter.formats.ksplat.KSplatFormat.write`` to formats/ksplat_writer.py:write_ksplat (SH-degree
    scan, bucket centres and every row on the GPU; identical file bytes).  A reference without that module is left as it is.
    splat_writer: also rebind ``gsconverter.formats.splat.SplatFormat.write`` to formats/splat_writer.py:write_splat (metric, sort
    and every record on the GPU; the reference's records, equal metrics kept in input order).  A reference without that module
    is left as it is.
    cply_reader: also rebind ``gsconverter.formats.compressed_ply.CompressedPlyFormat.read`` to formats/compressed_ply_reader.py
    (the decode on the GPU, no plyfile; the reference's rows and ``self.metadata``).  Files the device path does not take -- no
    `chunk` element, ascii or big-endian bodies, list properties -- go to the reference's own read.  A reference without that
    module is left as it is.
    ksplat_reader: also rebind ``gsconverter.formats.ksplat.KSplatFormat.read`` to formats/ksplat_reader.py (header walk on the
    host, every row decoded on the GPU; the reference's rows, ``self.metadata`` and its exceptions on malformed files).  Files the
    device path does not take -- a section of SH degree above 3, thousands of section headers, rows broadcast against a single
    bucket assignment -- go to the reference's own read.  A reference without that module is left as it is.
    spz_reader: also rebind ``gsconverter.formats.spz.SpzFormat.read`` to formats/spz_reader.py (streamed inflate into page-locked
    staging and the header on the host, every row decoded on the GPU; the reference's rows and its exceptions on malformed
    files).  A file of SH degree above 3 goes to the reference's own read.  A reference without that module is left as it is.
    sog_reader: also rebind ``gsconverter.formats.sog.SogFormat.read`` to formats/sog_reader.py (the bundle, meta.json and the
    threaded WebP decode into page-locked staging on the host, every row decoded on the GPU; the reference's rows and its
    exceptions on malformed files).  A file whose meta.json the device path does not take -- bands outside 1 ... 3, a palette
    outside 1 ... 65 536, values of other types than the writer's -- goes to the reference's own read.  A reference without
    that module is left as it is.
    splat_reader: also rebind ``gsconverter.formats.splat.SplatFormat.read`` to formats/splat_reader.py (the file's size and the
    read into page-locked staging on the host, every row decoded on the GPU; the reference's rows and its exceptions on a
    missing path).  Every .splat file is taken.  A reference without that module is left as it is.  Unlike the other readers
    this one is OFF unless asked for: a plain install() has always left ``SplatFormat.read`` to the reference, callers and tests
    rely on that, and adding a reader changes no existing behaviour.
    ply_reader: also rebind ``gsconverter.formats.ply_3dgs.Ply3DGSFormat.read`` and ``gsconverter.formats.ply_cc.PlyCCFormat.read``
    to formats/ply_reader.py (header, name mapping and the non-vertex elements on the host, the row transcode on the GPU, no
    plyfile; the reference's rows and ``self.extra_elements``).  Files the device path does not take -- ascii bodies, list
    properties, a duplicated vertex property, colours that are not uchar, big-endian files with extra fields, rows over 512
    bytes or 128 fields -- go to the reference's own read when plyfile is there.  A reference without those modules is left as
    it is.
    ply_writer: also rebind ``gsconverter.formats.ply_3dgs.Ply3DGSFormat.write`` and ``gsconverter.formats.ply_cc.PlyCCFormat.write``
    to formats/ply_writer.py (the output layout and the container on the host, the crop_sh scan and the row pack on the GPU, no
    plyfile; the reference's file byte for byte, `crop_sh` and `extra_elements` honoured).  Tables the device path does not take
    -- a field that is no PLY scalar, a big-endian field, rows over 512 bytes, more than 128 runs -- go to the reference's own
    write when plyfile is there.  A reference without those modules, or whose classes have no `write`, is left as it is.
    parquet_reader: also rebind ``gsconverter.formats.parquet.ParquetFormat.read`` to formats/parquet_reader.py (pyarrow's decode
    of the columns the rows use on the host, the columns -> rows transpose with numpy's casts and the validity bitmaps on the
    GPU; the reference's rows).  Files the device path does not take -- two columns on one output name, a needed column of
    another type than the integers and floats, a needed integer column with nulls, a stored index column -- go to the
    reference's own read.  OFF unless asked for, like splat_reader and for its reason: a plain install() has always left
    ``ParquetFormat`` to the reference, callers and tests on machines without a GPU rely on that.
    parquet_writer: also rebind ``gsconverter.formats.parquet.ParquetFormat.write`` to formats/parquet_writer.py (the rows ->
    columns transpose, the validity bitmaps and the null counts on the GPU, pyarrow's own write_table behind them; the
    reference's file byte for byte under the same pyarrow and pandas).  Tables the device path does not take -- a field that is
    none of f4, f8 and the integers, two fields on one column name, rows over 512 bytes or 128 fields -- go to the reference's
    own write.  OFF unless asked for, as parquet_reader is."""
    from . import processing
    from .processing import gpu_ops
    # the orchestrator ignores the filters' return values (converter.py:196-236), so ITS name gets the lazy class (coordinates
    # stay in HBM across filters); the public names keep the eager class, whose methods return self.data like the reference's
    from .processing.data_processor import ChainedDataProcessor, DataProcessor
    import gsconverter.processing as rp  # type: ignore  (raises ImportError if the reference is absent)
    import gsconverter.processing.data_processor as rdp  # type: ignore
    from .processing import data_processor as mine
    if rdp.DataProcessor is not DataProcessor and rdp.DataProcessor.__module__.startswith("gsconverter"):
        mine._REFERENCE_CLASS = rdp.DataProcessor  # methods with no device implementation are forwarded to it
    targets = [(rp, "DataProcessor", DataProcessor), (rdp, "DataProcessor", DataProcessor),
               (rp, "gpu_ops", gpu_ops)]
    for modname, attr, val in (("gsconverter.converter", "DataProcessor", ChainedDataProcessor),
                               ("gsconverter.formats.sog", "gpu_ops", gpu_ops)):
        try:
            targets.append((importlib.import_module(modname), attr, val))
        except ImportError:
            pass  # plyfile / pillow missing: that module of the REFERENCE is not importable, nothing to rebind
    for mod, attr, val in targets:
        _saved.setdefault((mod.__name__, attr), getattr(mod, attr, None))
        setattr(mod, attr, val)
    if sog_writer:
        # only the REFERENCE's module may be missing (pillow / plyfile absent: its own writer cannot run either);
        # a failure importing this package's writers propagates -- no silent return to the CPU writer
        try:
            sogmod = importlib.import_module("gsconverter.formats.sog")
        except ImportError:
            sogmod = None
        if sogmod is not None:
            from .formats.sog_writer import write_sog
            _saved.setdefault(("sogformat", "write"), sogmod.SogFormat.write)
            sogmod.SogFormat.write = lambda self, data, path, **kw: write_sog(data, path, **kw)
        try:
            cpmod = importlib.import_module("gsconverter.formats.compressed_ply")
        except ImportError:
            cpmod = None
        if cpmod is not None:
            from .formats.compressed_ply_writer import write_compressed_ply
            _saved.setdefault(("cplyformat", "write"), cpmod.CompressedPlyFormat.write)
            cpmod.CompressedPlyFormat.write = lambda self, data, path, **kw: write_compressed_ply(data, path, **kw)
    if spz_writer:
        try:
            spzmod = importlib.import_module("gsconverter.formats.spz")
        except ImportError:
            spzmod = None
        if spzmod is not None:
            from .formats.spz_writer import write_spz
            _saved.setdefault(("spzformat", "write"), spzmod.SpzFormat.write)
            spzmod.SpzFormat.write = lambda self, data, path, **kw: write_spz(data, path, **kw)
    if ksplat_writer:
        try:
            ksmod = importlib.import_module("gsconverter.formats.ksplat")
        except ImportError:
            ksmod = None
        if ksmod is not None:
            from .formats.ksplat_writer import write_ksplat
            _saved.setdefault(("ksplatformat", "write"), ksmod.KSplatFormat.write)
            ksmod.KSplatFormat.write = lambda self, data, path, compression_level=0, **kw: write_ksplat(data, path, compression_level, **kw)
    if splat_writer:
        try:
            spmod = importlib.import_module("gsconverter.formats.splat")
        except ImportError:
            spmod = None
        if spmod is not None:
            from .formats.splat_writer import write_splat
            _saved.setdefault(("splatformat", "write"), spmod.SplatFormat.write)
            spmod.SplatFormat.write = lambda self, data, path, **kw: write_splat(data, path, **kw)
    if cply_reader:
        try:
            cpmod = importlib.import_module("gsconverter.formats.compressed_ply")
        except ImportError:
            cpmod = None
        if cpmod is not None and getattr(cpmod.CompressedPlyFormat, "read", None) is not None:
            from .formats.compressed_ply_reader import bind_read
            _saved.setdefault(("cplyformat", "read"), cpmod.CompressedPlyFormat.read)
            cpmod.CompressedPlyFormat.read = bind_read(_saved[("cplyformat", "read")])
    if ksplat_reader:
        try:
            ksmod = importlib.import_module("gsconverter.formats.ksplat")
        except ImportError:
            ksmod = None
        if ksmod is not None and getattr(ksmod.KSplatFormat, "read", None) is not None:
            from .formats.ksplat_reader import bind_read as bind_ksplat_read
            _saved.setdefault(("ksplatformat", "read"), ksmod.KSplatFormat.read)
            ksmod.KSplatFormat.read = bind_ksplat_read(_saved[("ksplatformat", "read")])
    if spz_reader:
        try:
            spzmod = importlib.import_module("gsconverter.formats.spz")
        except ImportError:
            spzmod = None
        if spzmod is not None and getattr(spzmod.SpzFormat, "read", None) is not None:
            from .formats.spz_reader import bind_read as bind_spz_read
            _saved.setdefault(("spzformat", "read"), spzmod.SpzFormat.read)
            spzmod.SpzFormat.read = bind_spz_read(_saved[("spzformat", "read")])
    if sog_reader:
        try:
            sogmod = importlib.import_module("gsconverter.formats.sog")
        except ImportError:
            sogmod = None
        if sogmod is not None and getattr(sogmod.SogFormat, "read", None) is not None:
            from .formats.sog_reader import bind_read as bind_sog_read
            _saved.setdefault(("sogformat", "read"), sogmod.SogFormat.read)
            sogmod.SogFormat.read = bind_sog_read(_saved[("sogformat", "read")])
    if splat_reader:
        try:
            spmod = importlib.import_module("gsconverter.formats.splat")
        except ImportError:
            spmod = None
        if spmod is not None and getattr(spmod.SplatFormat, "read", None) is not None:
            from .formats.splat_reader import bind_read as bind_splat_read
            _saved.setdefault(("splatformat", "read"), spmod.SplatFormat.read)
            spmod.SplatFormat.read = bind_splat_read(_saved[("splatformat", "read")])
    if ply_reader:
        from .formats import ply_reader as plyr
        for key, modname, cls, bind in (("ply3dgsformat", "gsconverter.formats.ply_3dgs", "Ply3DGSFormat", plyr.bind_read_3dgs),
                                        ("plyccformat", "gsconverter.formats.ply_cc", "PlyCCFormat", plyr.bind_read_cc)):
            try:
                plymod = importlib.import_module(modname)
            except ImportError:
                plymod = None
            if plymod is not None and getattr(getattr(plymod, cls, None), "read", None) is not None:
                _saved.setdefault((key, "read"), getattr(plymod, cls).read)
                getattr(plymod, cls).read = bind(_saved[(key, "read")])
    if ply_writer:
        from .formats import ply_writer as plyw
        for key, modname, cls, bind in (("ply3dgsformat", "gsconverter.formats.ply_3dgs", "Ply3DGSFormat", plyw.bind_write_3dgs),
                                        ("plyccformat", "gsconverter.formats.ply_cc", "PlyCCFormat", plyw.bind_write_cc)):
            try:
                plymod = importlib.import_module(modname)
            except ImportError:
                plymod = None
            if plymod is not None and getattr(getattr(plymod, cls, None), "write", None) is not None:
                _saved.setdefault((key, "write"), getattr(plymod, cls).write)
                getattr(plymod, cls).write = bind(_saved[(key, "write")])
    if parquet_reader or parquet_writer:
        try:
            pqmod = importlib.import_module("gsconverter.formats.parquet")
        except ImportError:
            pqmod = None
        if pqmod is not None and parquet_reader and getattr(pqmod.ParquetFormat, "read", None) is not None:
            from .formats.parquet_reader import bind_read as bind_parquet_read
            _saved.setdefault(("parquetformat", "read"), pqmod.ParquetFormat.read)
            pqmod.ParquetFormat.read = bind_parquet_read(_saved[("parquetformat", "read")])
        if pqmod is not None and parquet_writer and getattr(pqmod.ParquetFormat, "write", None) is not None:
            from .formats.parquet_writer import bind_write as bind_parquet_write
            _saved.setdefault(("parquetformat", "write"), pqmod.ParquetFormat.write)
            pqmod.ParquetFormat.write = bind_parquet_write(_saved[("parquetformat", "write")])
    _saved.setdefault(("sys.modules", "gsconverter.processing.gpu_ops"),
                      sys.modules.get("gsconverter.processing.gpu_ops"))
    sys.modules["gsconverter.processing.gpu_ops"] = gpu_ops
    return processing


def uninstall():
    for (modname, attr), val in list(_saved.items()):
        if modname == "sogformat":
            setattr(importlib.import_module("gsconverter.formats.sog").SogFormat, attr, val)
            continue
        if modname == "cplyformat":
            setattr(importlib.import_module("gsconverter.formats.compressed_ply").CompressedPlyFormat, attr, val)
            continue
        if modname == "spzformat":
            setattr(importlib.import_module("gsconverter.formats.spz").SpzFormat, attr, val)
            continue
        if modname == "ksplatformat":
            setattr(importlib.import_module("gsconverter.formats.ksplat").KSplatFormat, attr, val)
            continue
        if modname == "splatformat":
            setattr(importlib.import_module("gsconverter.formats.splat").SplatFormat, attr, val)
            continue
        if modname == "ply3dgsformat":
            setattr(importlib.import_module("gsconverter.formats.ply_3dgs").Ply3DGSFormat, attr, val)
            continue
        if modname == "plyccformat":
            setattr(importlib.import_module("gsconverter.formats.ply_cc").PlyCCFormat, attr, val)
            continue
        if modname == "parquetformat":
            setattr(importlib.import_module("gsconverter.formats.parquet").ParquetFormat, attr, val)
            continue
        if modname == "sys.modules":
            if val is None:
                sys.modules.pop(attr, None)
            else:
                sys.modules[attr] = val
        elif val is not None:
            setattr(importlib.import_module(modname), attr, val)
    _saved.clear()
