"""Host arrays as device tensors in the forms the raw entry points take (test infrastructure only)."""
import numpy as np


def dev_u32(a):
    """uint32 counts as an int32 tensor on the device"""
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32), device="cuda")


def dev_coff(N):
    """the customers per restaurant as their I + 1 prefix sums (int64 holding uint64), the objects' d_coff"""
    import torch

    return torch.as_tensor(np.concatenate([[0], np.cumsum(N, dtype=np.int64)]), device="cuda")
