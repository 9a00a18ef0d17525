"""EEG preprocessing (reference: open_clip/modal_eeg/processors/eeg_processor.py:229-247 `EEGProcessorEval`): a
[channels, time] recording is cut to the window [time_low, time_high) and linearly resampled to `data_len` points per
channel (scipy `interp1d` over a [0, 1] grid in the reference).  128 x 512 values per sample: host-side data plumbing,
done here with the same two-point formula in numpy (pinned against scipy in tests/test_preproc_host.py); the result is
the [channels, data_len] float32 tensor the EEG tokenizer (PatchEmbed1D) takes.  `EEG_Processor` is the training-side name of the
same arithmetic; the paired image of a training sample goes through `Image_Processor_Train` (on the GPU, shared with the
tactile recipe: modal_tactile/processors/tact_processor.py)."""
import numpy as np
import torch

from open_clip.modal_tactile.processors.tact_processor import Image_Processor_Train  # noqa: F401  (the EEG recipe's paired image)


class BaseProcessor:
    def __init__(self):
        self.transform = lambda x: x

    def __call__(self, item):
        return self.transform(item)

    @classmethod
    def from_config(cls, cfg=None):
        return cls()

    def build(self, **kwargs):
        return self.from_config(dict(kwargs))


def linear_resample(y, n_out):
    """scipy.interpolate.interp1d(linspace(0, 1, T), y)(linspace(0, 1, n_out)) along the last axis (linear, float64)."""
    T = y.shape[-1]
    x, xn = np.linspace(0, 1, T), np.linspace(0, 1, n_out)
    hi = np.clip(np.searchsorted(x, xn), 1, T - 1)
    lo = hi - 1
    slope = (y[..., hi] - y[..., lo]) / (x[hi] - x[lo])
    return slope * (xn - x[lo]) + y[..., lo]


class EEGProcessorEval(BaseProcessor):
    def __init__(self, time_low=20, time_high=460, data_len=512):
        self.time_low, self.time_high, self.data_len = time_low, time_high, data_len

    def __call__(self, eeg):
        """eeg: path of a torch-saved [channels, time] tensor, or the tensor / array itself -> [channels, data_len]."""
        if isinstance(eeg, (str, bytes)) or hasattr(eeg, "__fspath__"):
            eeg = torch.load(eeg, map_location="cpu", weights_only=False)
        eeg = np.asarray(eeg.float().cpu() if isinstance(eeg, torch.Tensor) else eeg, dtype=np.float32)
        eeg = eeg[:, self.time_low:self.time_high]
        return torch.from_numpy(linear_resample(eeg, self.data_len)).float()


eeg_conf = {"time_low": 20, "time_high": 460, "data_len": 512}


class EEG_Processor(EEGProcessorEval):
    """The training-side processor (reference :196-226): the same window and resampling as `EEGProcessorEval`, configured by
    an argument object or mapping with `time_low`, `time_high`, `data_len`.  As in the reference the three values are read
    from `args` BEFORE `update_conf` is merged into it, so `update_conf` does not reach them."""

    def __init__(self, args=None, update_conf=None):
        conf = dict(eeg_conf)
        if args is not None:
            conf.update(args if hasattr(args, "keys") else {k: getattr(args, k) for k in conf if hasattr(args, k)})
        super().__init__(conf["time_low"], conf["time_high"], conf["data_len"])

    @classmethod
    def from_config(cls, cfg=None):
        cfg = dict(cfg or {})
        update_conf = cfg.pop("update_conf", None)
        return cls(args=cfg.get("params", eeg_conf), update_conf=update_conf)
