"""Gradient compression — mirrors tips/tensorflow/compression.py:20-75.

Compression.fp16 is usable here: the device path has an fp16 allreduce
(dtype code 4), whereas the reference casts to tf.float16 and then hits the
op's {int32, int64, float32, float64} constraint (ops.cc:121).
"""
import numpy as np

from . import tensors


class Compressor(object):
    """Interface for compressing and decompressing a given tensor (compression.py:20-31)."""

    @staticmethod
    def compress(tensor):
        pass

    @staticmethod
    def decompress(tensor, ctx):
        pass


class NoneCompressor(Compressor):
    """Default no-op compression (compression.py:34-46)."""

    @staticmethod
    def compress(tensor):
        return tensor, None

    @staticmethod
    def decompress(tensor, ctx):
        return tensor


def _is_floating(t):
    if tensors.is_torch(t):
        return t.dtype.is_floating_point
    return np.issubdtype(np.asarray(t).dtype, np.floating)


class FP16Compressor(Compressor):
    """Cast floating tensors to 16-bit for the wire (compression.py:49-66)."""

    @staticmethod
    def compress(tensor):
        compressed = tensor
        if _is_floating(tensor):
            if tensors.is_torch(tensor):
                import torch
                compressed = tensor.to(torch.float16)
            else:
                compressed = np.asarray(tensor).astype(np.float16)
        return compressed, tensor.dtype

    @staticmethod
    def decompress(tensor, ctx):
        if ctx is None or not _is_floating(tensor):
            return tensor
        if tensors.is_torch(tensor):
            return tensor.to(ctx)
        return np.asarray(tensor).astype(ctx)


class MXFP8Compressor(Compressor):
    """Block-scaled 8-bit wire. A marker, not a cast: an (8-bit payload, scales) pair
    cannot pass through a sum allreduce, so compress / decompress are the identity, and allreduce /
    allreduce_grads recognise the class and send float32 device tensors through the quantised
    collective (ops.allreduce_mxfp8 / ops.fused_allreduce_mxfp8). Every other tensor - host, another
    dtype, sparse - travels uncompressed, exactly as under Compression.none."""

    @staticmethod
    def compress(tensor):
        return tensor, None

    @staticmethod
    def decompress(tensor, ctx):
        return tensor

    @staticmethod
    def error_feedback():
        """A new stateful compressor for one gradient list: the MXFP8 wire with error feedback."""
        return MXFP8ErrorFeedback()


class MXFP8ErrorFeedback(Compressor):
    """The MXFP8 wire with error feedback: Compression.fp8.error_feedback(). An object,
    not a class - it owns the residuals that one gradient list carries from step to step: what the
    sender's quantiser and the chunk owner's requantiser dropped is added to the next step's input, so
    that the sum of T steps' outputs differs from the true sum by one bounded residual.

    allreduce_grads / DistributedOptimizer keep one zero-initialised float32 state tensor per
    (device, counts tuple, size()) - a new signature gets fresh zeros; allreduce(t, name=...) keeps
    one per (name, numel, device). Everything that is not a dense float32 device tensor travels as
    under Compression.fp8 (compress / decompress are the identity). reset() drops every state;
    state_dict() / load_state_dict() carry them through a checkpoint, keyed by signature. The states
    differ per rank: every rank saves and loads its own."""

    def __init__(self):
        self._states = {}

    def compress(self, tensor):
        return tensor, None

    def decompress(self, tensor, ctx):
        return tensor

    def _state(self, key, device, nbytes):
        """The state tensor of a signature on `device`: the stored one, or fresh zeros when there is
        none or its size is not what the call needs (a state of another rank count)."""
        import torch
        t = self._states.get(key)
        if t is None or t.numel() * 4 != nbytes or t.dtype != torch.float32:
            t = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)
        elif t.device != device:  # (loaded from a checkpoint held elsewhere)
            t = t.to(device)
        self._states[key] = t
        return t

    def list_state(self, device, counts, nranks):
        """The state of a gradient list: float32 [tips_mxfp8_ef_bytes(E, nranks) / 4] on `device`."""
        from . import ops
        counts = tuple(int(c) for c in counts)
        elems, _ = ops.mxfp8_flat_elems(list(counts))
        return self._state(("list", str(device), counts, int(nranks)), device, ops.mxfp8_ef_bytes(elems, nranks))

    def tensor_state(self, name, numel, device, nranks):
        """The state of allreduce(t, compression=self, name=name)."""
        from . import ops
        elems, _ = ops.mxfp8_flat_elems([int(numel)])
        return self._state(("tensor", str(name), int(numel), str(device)), device, ops.mxfp8_ef_bytes(elems, nranks))

    def reset(self):
        """Forget every residual: the next step of every signature starts from zeros."""
        self._states = {}

    def state_dict(self):
        """{signature: float32 tensor (a copy)} - what a checkpoint of this rank holds."""
        return {k: t.detach().clone() for k, t in self._states.items()}

    def load_state_dict(self, state):
        """Replace every state by copies of `state`'s tensors (a state_dict() of the same rank, rank
        count and gradient list); a tensor held on another device moves at its first use."""
        import torch
        new = {}
        for k, t in state.items():
            if not (isinstance(k, tuple) and k and k[0] in ("list", "tensor")):
                raise ValueError("not a signature of MXFP8ErrorFeedback.state_dict(): %r" % (k,))
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1):
                raise ValueError("the state of %r is not a flat float32 tensor" % (k,))
            new[k] = t.detach().clone()
        self._states = new


class Compression(object):
    """Optional gradient compression algorithm used during allreduce (compression.py:69-75)."""
    none = NoneCompressor
    fp16 = FP16Compressor
    fp8 = MXFP8Compressor
