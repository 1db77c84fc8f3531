"""mdm -- MI355X-native masked-diffusion train step and reverse sampler.

Host side (Python on PyTorch-ROCm for device memory / streams / torch.distributed)
over libmdm_hip.so (hand-written HIP kernels for gfx950, C ABI in include/mdm_hip.h, image grids in
include/mdm_vis.h, the device-resident data set in include/mdm_data.h, image-folder ingest in
include/mdm_ingest.h, nearest-neighbour search in include/mdm_neighbor.h, the inpainting sampler in
include/mdm_inpaint.h, image quality in include/mdm_metric.h, the restoration sampler in
include/mdm_restore.h, set moments and the Frechet distance in include/mdm_moment.h).
Keeps the reference's call surface: Scheduler(args), Sampler(dataset, args, Scheduler,
dataset_hist).sample(model, timesteps), Trainer(...).train(...), model(x, t).sample.
"""
from . import _lib  # noqa: F401
from . import evaluate  # noqa: F401
from . import ingest  # noqa: F401
from . import metrics  # noqa: F401
from . import moments  # noqa: F401
from . import rawsets  # noqa: F401
from . import visuals  # noqa: F401
from ._lib import BF16, F32  # noqa: F401
from .data import DeviceDataset, DeviceLoader  # noqa: F401
from .dist import GradComm  # noqa: F401
from .evaluate import NeighborBank, get_nearest_neighbor, get_nearest_neighbor_idx, get_similar_neighbor  # noqa: F401
from .metrics import ImageMetrics, image_metrics, mean_fill_baseline  # noqa: F401
from .moments import FrechetResult, MomentPlan, SetMoments, frechet_distance, moment_plan, moment_tile_of  # noqa: F401
from .ingest import get_dataset, image_folder, ingest_block, resize_crop_plan  # noqa: F401
from .optim import EMA, SGD, Accelerator, Adam, AdamW, get_lr_scheduler, get_optimizer  # noqa: F401
from .rawsets import cifar10_arrays, flowers102_samples, mnist_arrays, read_idx  # noqa: F401
from .sampler import Sampler, inpaint_keep, inpaint_start_index, restore_expand, restore_measure  # noqa: F401
from .scheduler import Scheduler  # noqa: F401
from .train_step import MonitorRing  # noqa: F401
from .trainer import BaseTrainer, Trainer  # noqa: F401
from .unet import UNet, unet6_config  # noqa: F401
from .unet2d import UNet2D, my_model_config  # noqa: F401
