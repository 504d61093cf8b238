"""Writers whose numeric core runs on the MI355X: the SOG bundle, the compressed PLY and the 3DGS / CloudCompare PLY."""
from .sog_writer import write_sog  # noqa: F401
from .compressed_ply_writer import write_compressed_ply  # noqa: F401
from .ply_writer import write_ply_3dgs, write_ply_cc  # noqa: F401
