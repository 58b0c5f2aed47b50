"""The critic of AtcVecEnv.value_forward and AtcVecEnv.ppo_value_grad (include/atc_step.h: atc_value_forward, atc_ppo_value_grad) as the
library reads it: one float32 array of L.value_words(K) words — W1[64][10 + 7 K], b1[64], W2[64][64], b2[64], W3[1][64], b3[1], every weight
matrix row-major [out][in], i.e. torch.nn.Linear.weight as it lies in memory.  This is atc_hip.policy's packing without the two further rows
of its head and without log_std; the critic reads the same input row as the policy: the own row, then words 0..6 of each of the K traffic
records (atc_hip.policy.input_rows)."""
from . import layout as L

SHAPES = (("W1", (L.POLICY_HIDDEN, L.POLICY_IN)), ("b1", (L.POLICY_HIDDEN,)), ("W2", (L.POLICY_HIDDEN, L.POLICY_HIDDEN)), ("b2", (L.POLICY_HIDDEN,)),
          ("W3", (1, L.POLICY_HIDDEN)), ("b3", (1,)))


def shapes(traffic=0):
    """SHAPES with the first layer of a critic that sees `traffic` records per aircraft"""
    if traffic not in (0,) + L.POLICY_TRAFFIC_K:
        raise ValueError("traffic must be 0 or one of %s records per aircraft" % (L.POLICY_TRAFFIC_K,))
    return (("W1", (L.POLICY_HIDDEN, L.policy_in(traffic))),) + SHAPES[1:]


def offsets(traffic=0):
    """{name: (first word, shape)} of the six parts of the packed array"""
    out, at = {}, 0
    for name, shape in shapes(traffic):
        n = 1
        for s in shape:
            n *= s
        out[name] = (at, shape)
        at += n
    assert at == L.value_words(traffic)
    return out


def pack_mlp(W1, b1, W2, b2, W3, b3, device=None, traffic=0):
    """The value_words(traffic)-word float32 tensor of an IN -> 64 -> 64 -> 1 MLP, IN = 10 + 7 traffic, with weights [out, in] (tensors or
    arrays; shapes are checked, nothing is transposed or broadcast).  On `device` (default: the first part's device if it is a tensor,
    else the CPU): value_forward and ppo_value_grad need it on the env's device."""
    import torch
    parts = []
    for (name, shape), v in zip(shapes(traffic), (W1, b1, W2, b2, W3, b3)):
        t = torch.as_tensor(v).detach()
        if tuple(t.shape) != shape:
            raise ValueError("%s must have shape %s (weights are [out, in]), got %s" % (name, shape, tuple(t.shape)))
        if device is None and t.is_cuda:
            device = t.device
        parts.append(t)
    flat = torch.cat([t.to(device=device or "cpu", dtype=torch.float32).reshape(-1) for t in parts]).contiguous()
    assert flat.numel() == L.value_words(traffic)
    return flat


def traffic_of(words):
    """K of a packed critic of `words` floats; ValueError for any other size"""
    for K in (0,) + L.POLICY_TRAFFIC_K:
        if int(words) == L.value_words(K):
            return K
    raise ValueError("weights must hold %s words (atc_hip.value.pack_mlp with traffic = 0, 1, 2, 4), got %d" % (
        ", ".join(str(L.value_words(K)) for K in (0,) + L.POLICY_TRAFFIC_K), int(words)))


def unpack(w, traffic=None):
    """{name: view} of the six parts W1 .. b3 of the packed critic `w` (a tensor or an array of value_words(K) elements; K from its size, or
    `traffic`, which must agree), each in its shape [out, in].  Views: writing to one writes to `w`."""
    flat = w.reshape(-1)
    n = int(flat.shape[0])
    K = traffic_of(n) if traffic is None else int(traffic)
    if n != L.value_words(K):
        raise ValueError("a critic with traffic=%d has %d words, got %d" % (K, L.value_words(K), n))
    out = {}
    for name, (at, shape) in offsets(K).items():
        size = 1
        for s in shape:
            size *= s
        out[name] = flat[at:at + size].reshape(shape)
    return out


def to_torch(w, traffic=None):
    """nn.Sequential(Linear(10 + 7 K, 64), Tanh(), Linear(64, 64), Tanh(), Linear(64, 1)) holding COPIES of the packed critic `w`, float32, on
    w's device: the inverse of from_torch — from_torch(to_torch(w), traffic=K) gives back `w` bit for bit."""
    import torch
    from torch import nn
    p = unpack(torch.as_tensor(w).detach(), traffic)
    n_in = int(p["W1"].shape[1])
    net = nn.Sequential(nn.Linear(n_in, L.POLICY_HIDDEN), nn.Tanh(), nn.Linear(L.POLICY_HIDDEN, L.POLICY_HIDDEN), nn.Tanh(),
                        nn.Linear(L.POLICY_HIDDEN, 1)).to(device=p["W1"].device, dtype=torch.float32)
    with torch.no_grad():
        for lin, (wn, bn) in zip(list(net)[0::2], (("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
            lin.weight.copy_(p[wn])
            lin.bias.copy_(p[bn])
    return net


def from_torch(module, device=None, traffic=0):
    """pack_mlp of an nn.Sequential(Linear(10 + 7 traffic, 64), Tanh(), Linear(64, 64), Tanh(), Linear(64, 1)) — biases required."""
    from torch import nn
    layers = list(module)
    kinds = (nn.Linear, nn.Tanh, nn.Linear, nn.Tanh, nn.Linear)
    if len(layers) != len(kinds) or not all(isinstance(m, k) for m, k in zip(layers, kinds)):
        raise ValueError("need nn.Sequential(Linear, Tanh, Linear, Tanh, Linear)")
    lin = layers[0::2]
    if any(m.bias is None for m in lin):
        raise ValueError("every Linear layer needs a bias")
    return pack_mlp(lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias, device=device, traffic=traffic)
