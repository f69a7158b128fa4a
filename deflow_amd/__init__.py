"""deflow_amd -- MI355X-native DeFlow scene-flow hot path (HIP kernels behind the reference's model plugin API)."""
from .deflow import DeFlow, cal_pose0to1  # noqa: F401
from .encoder import DynamicEmbedder  # noqa: F401
from .unet import ConvWithNorms, FastFlow3DUNet  # noqa: F401
from .decoder import ConvGRU, ConvGRUDecoder, LinearDecoder  # noqa: F401
from .timer import Timing  # noqa: F401
from .cluster import dbscan, dynamic_cluster_labels  # noqa: F401
from .voidmap import VoidMap, label_scene  # noqa: F401
from .ground import GroundSegmenter  # noqa: F401
from .metrics_device import DeviceMetrics  # noqa: F401
from .sweeps import SweepFlow  # noqa: F401
from .submit import SubmitFlow  # noqa: F401
from .augment import Augmenter  # noqa: F401
from .render import flow_vectors, render_rows  # noqa: F401
