"""MI355X-native ORB front-end (ORBextractor::operator() + Hamming matching) behind the C ABI of liborbx.so.

Python here is plumbing only: ctypes marshalling, torch.distributed sharding of frame batches, synthetic
inputs.  All compute is in csrc/ (hand-written HIP for gfx950).  There is no CPU fallback.
"""
from ._capi import KP_DTYPE, OrbxError, LIB_PATH  # noqa: F401
from .extractor import ORBextractor  # noqa: F401
from .matcher import ORBmatcher  # noqa: F401
from .frame import Frame, depth_map_factor  # noqa: F401
from .vocabulary import ORBVocabulary  # noqa: F401
from .keyframe_db import KeyFrameDatabase, bow_score  # noqa: F401
from .mappoint import (distinctive_descriptors_batch, distinctive_descriptors_batch_device,  # noqa: F401
                       update_normal_and_depth_batch)
from .optimizer import optimize_essential_graph_batch, optimize_sim3_batch, pose_optimization, pose_optimization_batch  # noqa: F401
from .sim3 import (Sim3Ransac, compute_sim3_round_robin, compute_sim3_rounds_batched, compute_sim3_rounds_device,  # noqa: F401
                   ransac_iterations)
from .pnp import PnPRansac, relocalization_round_robin, pnp_ransac_parameters  # noqa: F401
from .initializer import InitializerRansac, InitializerReconstruct, initialize_batch, INIT_NONE, INIT_H, INIT_F  # noqa: F401
from .localmapping import create_new_map_points_batch, create_new_map_points_rounds  # noqa: F401
from .loopclosing import essential_graph_edges, sim3_from_Tcw  # noqa: F401
