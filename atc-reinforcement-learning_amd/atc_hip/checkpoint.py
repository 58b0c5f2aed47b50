"""A packed policy (atc_hip.policy) and, optionally, a packed critic (atc_hip.value) as a plain .npz file: the named parts of each as float32
arrays ("policy/W1" .. "policy/log_std", "value/W1" .. "value/b3"), the traffic records per aircraft each was packed for ("policy/traffic",
"value/traffic") and the caller's meta data as one JSON string ("meta").  No pickle: the file loads with numpy.load(allow_pickle=False), and
what comes back from load() is bit for bit what save() was given."""
import json

import numpy as np

from . import policy, value

FORMAT = 1


def _host(w):
    """the float32 numpy copy of a packed tensor or array"""
    if hasattr(w, "detach"):
        w = w.detach().cpu().numpy()
    w = np.ascontiguousarray(w)
    if w.dtype != np.float32:
        raise ValueError("packed weights are float32, got %s" % w.dtype)
    return w.reshape(-1)


def save(path, w, vw=None, **meta):
    """Writes the packed policy `w` and the packed critic `vw` (or None) to `path` (a name or an open binary file; numpy appends ".npz" to
    a name without it).  meta: anything json.dumps takes — the trainer's step count, the sector's name, the sim parameters."""
    arrays = {"format": np.int64(FORMAT), "meta": np.array(json.dumps(meta, sort_keys=True))}
    for prefix, mod, packed in (("policy", policy, w), ("value", value, vw)):
        if packed is None:
            continue
        flat = _host(packed)
        K = mod.traffic_of(flat.size)
        arrays[prefix + "/traffic"] = np.int64(K)
        for name, part in mod.unpack(flat, K).items():
            arrays[prefix + "/" + name] = part
    np.savez(path, **arrays)


def load(path, device=None):
    """{"policy": the packed policy, "value": the packed critic or None, "traffic": the policy's K, "value_traffic": the critic's K or None,
    "meta": dict} of a file save() wrote.  The packed arrays are float32 torch tensors on `device` (default: the CPU)."""
    import torch
    with np.load(path, allow_pickle=False) as z:
        if int(z["format"]) != FORMAT:
            raise ValueError("not a checkpoint of format %d" % FORMAT)
        out = {"meta": json.loads(str(z["meta"])), "value": None, "value_traffic": None}
        for prefix, mod, key, key_k in (("policy", policy, "policy", "traffic"), ("value", value, "value", "value_traffic")):
            if prefix + "/traffic" not in z.files:
                continue
            K = int(z[prefix + "/traffic"])
            parts = [z[prefix + "/" + name] for name, _ in mod.shapes(K)]
            out[key] = mod.pack_mlp(*parts, device=device or "cpu", traffic=K)
            out[key_k] = K
    if "policy" not in out:
        raise ValueError("the file holds no policy")
    return out
