"""What the train_*.py wrappers decide on the host, once: how a module of a reference-style model is swapped for its HIP twin, how
a module adopts another one's children, which arguments are refused before anything touches the library, and which tensors the
kernels read in place.

    swap_modules(model, make, name)            the traversal behind every use_hip_* call
    adopt(cls, old)                            a cls instance made of old's own children, Parameters and buffers
    is_real / is_number / check_number, check_tensor, check_f32, check_devices, check_grad      the argument checks
    rows_in_place(t, width, stride), aligned_copy(t)                                  the in-place-or-copy layout rule

Every check raises ValueError, except a tensor that is not on a GPU: MickeyHipError (there is no CPU fallback).  The message starts
with the public function's name and names the argument.
"""
import math
import numbers

import torch
from torch import nn

from . import _native


# ---- swapping modules ------------------------------------------------------------------------------------------------------
def swap_modules(model, make, name=None):
    """Replace, in place, every child module inside `model` for which make(child) returns a module (None = leave it alone) by that
    module; with `name`, only children registered under that name are looked at.  The modules are listed before the first swap, a
    module registered under several parents is made once and stays ONE module, and the old modules are kept referenced until the
    end, so that no new object can take the id of one already seen.  Returns the number of registrations replaced."""
    swapped = 0
    made = {}   # id(old) -> (old, new)
    for parent in list(model.modules()):
        for key, child in list(parent._modules.items()):
            if child is None or (name is not None and key != name):
                continue
            if id(child) not in made:
                new = make(child)
                if new is None:
                    continue
                made[id(child)] = (child, new)
            parent._modules[key] = made[id(child)][1]
            swapped += 1
    return swapped


def adopt(cls, old):
    """An instance of the nn.Module subclass `cls`, made without cls.__init__, that holds the very child modules, Parameters and
    buffers of `old` under the same names and in the same order, and old's training flag."""
    new = cls.__new__(cls)
    nn.Module.__init__(new)
    new._modules.update(old._modules)
    new._parameters.update(old._parameters)
    new._buffers.update(old._buffers)
    new._non_persistent_buffers_set = set(old._non_persistent_buffers_set)
    new.training = old.training
    return new


# ---- argument checks -------------------------------------------------------------------------------------------------------
def is_real(v):
    """A finite real number that is no bool."""
    return not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(float(v))


def is_number(v, positive=False):
    """A finite real number that is no bool and not negative (positive=True: greater than zero)."""
    return is_real(v) and (float(v) > 0 if positive else float(v) >= 0)


def check_number(fn, name, v, positive=False):
    if not is_number(v, positive):
        raise ValueError("%s: %s must be a finite %s number, got %r" % (fn, name, "positive" if positive else "non-negative", v))


def check_tensor(fn, name, t):
    if not torch.is_tensor(t):
        raise ValueError("%s: %s must be a tensor, got %s" % (fn, name, type(t).__name__))


def check_f32(fn, name, t, rank=None, width=None, shape=None, why=""):
    """t is a float32 tensor without an empty dimension and, where given, of that rank, that last dimension, that exact shape.
    `why` (e.g. what the op covers) ends the message about a wrong rank, width or shape."""
    check_tensor(fn, name, t)
    if t.dtype != torch.float32:
        raise ValueError("%s: %s must be float32, got %s (autocast is not covered)" % (fn, name, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s: %s must be %s, got %s%s" % (fn, name, tuple(shape), tuple(t.shape), why))
    if rank is not None and t.dim() != rank:
        raise ValueError("%s: %s must have %d dimensions, got %s%s" % (fn, name, rank, tuple(t.shape), why))
    if width is not None and (t.dim() < 1 or t.shape[-1] != width):
        raise ValueError("%s: the last dimension of %s must be %d, got %s%s" % (fn, name, width, tuple(t.shape), why))
    if t.numel() == 0:
        raise ValueError("%s: empty %s %s" % (fn, name, tuple(t.shape)))


def check_devices(fn, named):
    """named: [(argument name, tensor)].  All on a GPU (else MickeyHipError), and on the same one."""
    first = named[0][1].device
    if all(t.is_cuda and t.device == first for _, t in named):
        return
    where = ", ".join("%s on %s" % (n, t.device) for n, t in named)   # (only here: formatting a device costs a microsecond per tensor)
    if not all(t.is_cuda for _, t in named):
        raise _native.MickeyHipError("%s: needs device tensors (%s); mickey_amd has no CPU fallback" % (fn, where))
    raise ValueError("%s: tensors on different devices (%s)" % (fn, where))


def check_grad(fn, go):
    if go.dtype != torch.float32:
        raise ValueError("%s backward: the incoming gradient must be float32, got %s" % (fn, go.dtype))


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def rows_in_place(t, width, stride):
    """Whether the kernels can read rows of `width` elements that start `stride` elements apart where t holds them (the kernels'
    own MK_CHECK_ARG): the innermost dimension dense, the rows not overlapping and a multiple of 4 elements apart, the first one at a
    16-byte boundary."""
    return t.stride(-1) == 1 and stride >= width and stride % 4 == 0 and t.data_ptr() % 16 == 0


def aligned_copy(t):
    """t itself when it is contiguous and starts at a 16-byte boundary (a dense tensor may sit at an odd offset of its storage),
    else one contiguous copy, which does.  Differentiable."""
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)
