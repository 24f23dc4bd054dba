"""Checkpointing, logging, profiling helpers."""
from .checkpoint import (ModelCheckpoint, build_checkpoint, ema_entry, load_checkpoint,  # noqa: F401
                         load_model_state, save_checkpoint)
from .logging import CSVLogger, MultiLogger, TensorBoardLogger  # noqa: F401
