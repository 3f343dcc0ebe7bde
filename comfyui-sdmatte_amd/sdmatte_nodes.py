"""ComfyUI node `Apply SDMatte` + model-load API, MI355X-native.

Drop-in for /root/reference/sdmatte_nodes.py: same `SDMatteApply` class attributes and `apply_matte`
signature (sdmatte_nodes.py:217-257), same `NODE_CLASS_MAPPINGS` / `NODE_DISPLAY_NAME_MAPPINGS`
(:408-414), same module-level `MODEL_DIR`, `MODEL_URLS`, `download_model`, `ensure_sd21_from_manojb`
(:9-17,34,103).  What changes underneath:
  * the model is the hand-written HIP engine (engine.py -> libsdmatte_hip.so), not diffusers modules;
  * the built model is cached per (checkpoint path, mtime, device) instead of being rebuilt and re-read on every
    call (the reference does both per call, :286-323);
  * resize / normalise / forward / resize-back / clamp / `mask_refine` / output composition (:339-397) run on the GPU in
    one C-ABI call (`sdm_apply_matte_node`); `refine_and_compose` below is the same tail on CPU tensors, kept as the
    bit-exact restatement the tests compare with;
  * two nodes beyond the reference, registered only with SDMATTE_EXTRA_NODES=1 (the default surface stays the reference's):
    `SDMatteTrimapFromMask` makes the trimap from a mask on the GPU (the reference's README leaves "Create Trimap" to other nodes) and
    `SDMatteApplyMask` is `SDMatteApply` fed with a mask; `trimap_from_mask` below is the bit-exact CPU restatement of both;
  * one more node beyond the reference, registered only with SDMATTE_FOREGROUND_NODE=1: `SDMatteForeground` estimates the foreground and
    background colours from the image and the alpha on the GPU (clean cut-outs without the old background's halo); `estimate_foreground`
    below is its CPU restatement;
  * and one registered only with SDMATTE_REFINE_NODE=1: `SDMatteRefineAlpha` refines the alpha at the image's own resolution with the subsampled
    colour guided filter on the GPU (the model never sees more than `inference_size` pixels per side); `guided_refine_alpha` below is its torch
    restatement;
  * and one registered only with SDMATTE_ROI_NODE=1: `SDMatteApplyROI` is `SDMatteApplyMask` on the subject instead of the frame: the model is shown
    the box of the trimap at `inference_size` and its alpha is put back into the frame, all inside one engine call; `subject_roi` and `paste_roi`
    below are the exact CPU restatements of the box and of the way back;
  * and one registered only with SDMATTE_CANVAS_NODE=1: `SDMatteCanvas` frames a straight-alpha cut-out on a canvas of a given size (scaled, aligned,
    over a colour, an image or transparency, with an optional soft shadow), resampled premultiplied, in one engine call; `canvas_fit` is the exact
    restatement of its placement and `compose_canvas` its torch restatement;
  * and one registered only with SDMATTE_VIDEO_NODE=1: `SDMatteTemporalSmooth` takes the batch as a clip and filters the alpha along time, guided by
    the frames themselves, in one kernel launch; `temporal_smooth_alpha` below is its torch restatement;
  * and one registered only with SDMATTE_MOTION_NODE=1: `SDMatteTemporalSmoothMotion` is the same filter along a block-matched displacement, so the
    soft edge of a moving subject is smoothed too; `temporal_smooth_alpha_motion` below is its torch restatement;
  * and one registered only with SDMATTE_DEFOCUS_NODE=1: `SDMatteDefocus` puts the subject back over its own background out of focus (a normalised
    disc blur that does not see the subject, so no halo), in two kernel launches; `defocus_background` below is its torch restatement;
  * and one registered only with SDMATTE_HARMONIZE_NODE=1: `SDMatteHarmonize` sits the cut-out in a new scene (colour match in opponent coordinates,
    light wrap along the edge, then "over"), in one to four kernel launches; `harmonize_map` / `harmonize_cutout` below are its torch restatement;
  * and one registered only with SDMATTE_METRICS_NODE=1: `SDMatteMetrics` scores an alpha against a ground truth with the matting literature's SAD, MSE,
    Grad and Conn over the trimap's unknown band, on the GPU; `matte_metrics` below is its torch restatement;
  * and one registered only with SDMATTE_PLATE_NODE=1: `SDMatteCleanPlate` gives back the photo without its subject (the hole filled by push-pull from
    the background around it; background pixels come back bit for bit), in 1 + 2 ceil(S / 3) kernel launches; `clean_plate` below is its torch
    restatement;
  * and two registered only with SDMATTE_KEY_NODES=1, for green- and blue-screen shots: `SDMatteChromaKey` finds the screen's colour, keys the image
    against it (optionally against the screen's colour at each pixel, the clean plate of a first key) and returns the trimap for the model, the key,
    the despilled image and the screen; `SDMatteDespill` takes the screen's reflected light out of an image or a foreground; `screen_colour`,
    `chroma_key` and `key_screen` below are their torch restatements;
  * `force_cpu=True` is rejected: this node has no CPU path (the reference's own force_cpu branch cannot run either:
    meta_arch.py hard-codes `.cuda()`).
"""
import os
import threading

import torch

try:  # inside ComfyUI
    import folder_paths
except Exception:  # headless use (bench / tests): minimal stand-in with the three functions the node needs
    class _FolderPaths:
        def __init__(self):
            self.models_dir = os.environ.get("SDMATTE_MODELS_DIR", os.path.join(os.path.expanduser("~"), ".cache", "sdmatte_models"))
            self._paths = {}

        def add_model_folder_path(self, name, path):
            self._paths.setdefault(name, [])
            if path not in self._paths[name]:
                self._paths[name].append(path)

        def get_folder_paths(self, name):
            return list(self._paths.get(name, []))

    folder_paths = _FolderPaths()

try:
    import comfy.model_management as _comfy_mm
except Exception:
    _comfy_mm = None

MODEL_DIR = os.path.join(folder_paths.models_dir, "SDMatte")
folder_paths.add_model_folder_path("SDMatte", MODEL_DIR)

MODEL_URLS = {
    "SDMatte.safetensors": "https://huggingface.co/1038lab/SDMatte/resolve/main/SDMatte.safetensors",
    "SDMatte_plus.safetensors": "https://huggingface.co/1038lab/SDMatte/resolve/main/SDMatte_plus.safetensors",
}

# The reference needs these SD-2.1 config files to instantiate diffusers modules; the native engine embeds the constants
# (config.py) and never reads them.  The helper is kept so that callers of the reference API keep working.
SD21_MANOJB_FILES = {p: p for p in (
    "model_index.json", "text_encoder/config.json", "vae/config.json", "unet/config.json", "scheduler/scheduler_config.json",
    "tokenizer/tokenizer_config.json", "tokenizer/merges.txt", "tokenizer/vocab.json", "tokenizer/special_tokens_map.json",
    "feature_extractor/preprocessor_config.json")}


def _fetch(url, target):
    """Stream `url` to `target` through a .tmp file + atomic rename; verifies content-length when known."""
    os.makedirs(os.path.dirname(target), exist_ok=True)
    tmp = target + ".tmp"
    try:
        try:
            import requests
        except ImportError:
            import urllib.request
            urllib.request.urlretrieve(url, tmp)
        else:
            with requests.get(url, stream=True, timeout=60) as resp:
                resp.raise_for_status()
                expected = int(resp.headers.get("content-length", 0) or 0)
                with open(tmp, "wb") as fh:
                    for block in resp.iter_content(1 << 20):
                        if block:
                            fh.write(block)
                if expected and os.path.getsize(tmp) != expected:
                    raise IOError(f"[SDMatte] Incomplete download: {os.path.getsize(tmp)} != {expected}")
        if os.path.isfile(target) and os.path.getsize(target) > 0:   # someone else finished first
            os.remove(tmp)
        else:
            os.replace(tmp, target)
    except BaseException:
        if os.path.exists(tmp):
            try:
                os.remove(tmp)
            except OSError:
                pass
        raise
    return target


def ensure_sd21_from_manojb(sd21_base_dir=None):
    """API-compatible with the reference (sdmatte_nodes.py:34-101): make sure the SD-2.1 config files exist.
    Best effort (failures are printed, not raised); the native engine does not depend on the result."""
    if sd21_base_dir is None:
        roots = folder_paths.get_folder_paths("diffusers") or [os.path.join(folder_paths.models_dir, "diffusers")]
        sd21_base_dir = os.path.join(roots[0], "stable-diffusion-2-1-base")
    os.makedirs(sd21_base_dir, exist_ok=True)
    base = "https://huggingface.co/Manojb/stable-diffusion-2-1-base/resolve/main"
    for rel in SD21_MANOJB_FILES:
        dst = os.path.join(sd21_base_dir, rel)
        if os.path.isfile(dst):
            continue
        try:
            _fetch(f"{base}/{rel}", dst)
            print(f"[SDMatte] Downloaded {rel}")
        except Exception as exc:  # noqa: BLE001 - mirror the reference: warn and continue
            print(f"[SDMatte] Warning: failed to download {rel}: {exc}")
    return sd21_base_dir


def download_model(model_name, models_dir=MODEL_DIR, model_urls=MODEL_URLS):
    """Locate (every registered "SDMatte" folder first) or download a checkpoint; ValueError on unknown names
    (reference: sdmatte_nodes.py:103-199)."""
    for root in folder_paths.get_folder_paths("SDMatte") or []:
        cand = os.path.join(root, model_name)
        try:
            if os.path.isfile(cand) and os.path.getsize(cand) > 0:
                print(f"[SDMatte] Found model at: {cand}")
                return cand
        except OSError:
            continue
    url = model_urls.get(model_name)
    if not url:
        raise ValueError(f"[SDMatte] Unknown model name: {model_name}")
    target = os.path.join(models_dir, model_name)
    if os.path.isfile(target) and os.path.getsize(target) > 0:
        return target
    print(f"[SDMatte] Model '{model_name}' not found. Downloading to {target}...")
    _fetch(url, target)
    print(f"[SDMatte] Download complete: {target}")
    return target


SDMatteCore = None            # lazily bound, like the reference's module global (sdmatte_nodes.py:201,262-264)
_MODEL_CACHE = {}
_CACHE_LOCK = threading.Lock()


def _torch_device():
    if _comfy_mm is not None:
        return _comfy_mm.get_torch_device()
    if not torch.cuda.is_available():
        raise RuntimeError("[SDMatte] no ROCm GPU visible: the MI355X-native node has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


class LazyCheckpoint:
    """`state_dict`-like view of a .safetensors file that materialises ONE tensor at a time from the memory map (the engine packs
    every tensor into its own arena as it arrives; a dict of all tensors would hold the whole 3.8 GB checkpoint on the host).
    Only `text_encoder.*` is skipped up front: dead on this path (meta_arch.py:220-234 is never consumed, replace.py:414-416)."""

    def __init__(self, path):
        self.path = path

    def keys(self):
        from safetensors import safe_open
        with safe_open(self.path, framework="pt", device="cpu") as f:
            return [k for k in f.keys()]

    def items(self):
        from safetensors import safe_open
        with safe_open(self.path, framework="pt", device="cpu") as f:
            for key in f.keys():
                if key.startswith("text_encoder."):
                    continue
                yield key, f.get_tensor(key)


def load_checkpoint_state_dict(path):
    return LazyCheckpoint(path)


def get_model(ckpt_name, device):
    """Build (once) and cache the engine for (checkpoint file, mtime, device)."""
    global SDMatteCore
    if SDMatteCore is None:
        from .core import SDMatte as SDMatteCore
    path = download_model(ckpt_name)
    key = (os.path.realpath(path), os.path.getmtime(path), str(device))
    with _CACHE_LOCK:
        model = _MODEL_CACHE.get(key)
        if model is None:
            model = SDMatteCore(
                pretrained_model_name_or_path=None, load_weight=False, use_aux_input=True, aux_input="trimap",
                aux_input_list=["point_mask", "bbox_mask", "mask", "trimap"],
                attn_mask_aux_input=["point_mask", "bbox_mask", "mask", "trimap"],
                use_encoder_hidden_states=True, use_attention_mask=True, add_noise=False)
            model.load_state_dict(load_checkpoint_state_dict(path), strict=False)
            model.eval()
            model.to(device)
            _MODEL_CACHE.clear()          # one resident checkpoint per process is enough for the node
            _MODEL_CACHE[key] = model
    return model


def _trim_engine_memory(model):
    """The engine's activation arena lives outside torch's / ComfyUI's allocators and is sized by the largest call so far.  Give it
    back after the call when it is large (SDMATTE_KEEP_ARENA_GB, default 8), so that other nodes of the workflow can use the memory;
    the packed weights stay resident (that is the point of the model cache)."""
    try:
        limit = float(os.environ.get("SDMATTE_KEEP_ARENA_GB", "8")) * 2 ** 30
        engines = [model.engine] + (list(model._fan.engines[1:]) if getattr(model, "_fan", None) is not None else [])
        for eng in engines:
            if eng.resident_bytes() - eng.weight_bytes() > limit:      # arena + I/O staging only: ALL weight layouts stay
                eng.release_memory()
    except Exception as exc:  # noqa: BLE001 - best effort, like the reference's empty_cache block (sdmatte_nodes.py:399-403)
        print(f"[SDMatte] note: could not trim engine memory ({exc})")


def unload_models():
    """Drop the cached engine(s): every byte the node holds on the GPU is released."""
    with _CACHE_LOCK:
        for eng in _TRIMAP_ENGINES.values():
            eng.close()
        _TRIMAP_ENGINES.clear()
        for model in list(_MODEL_CACHE.values()):
            fan = getattr(model, "_fan", None)
            if fan is not None:
                fan.close()
            if model.engine is not None:
                model.engine.close()
        _MODEL_CACHE.clear()


_TRIMAP_ENGINES = {}          # device index -> weightless engine of SDMatteTrimapFromMask (under _CACHE_LOCK)


def _trimap_engine(device):
    """Engine for `make_trimap` on `device`: the resident cached model's if there is one on that device, otherwise a minimal context that is
    created once and kept (the tiny architecture, never loaded: sdm_make_trimap needs no weights, and no checkpoint is read or packed)."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    with _CACHE_LOCK:
        for model in _MODEL_CACHE.values():
            eng = getattr(model, "engine", None)
            if eng is not None and eng.h and eng.device == index:
                return eng
        eng = _TRIMAP_ENGINES.get(index)
        if eng is None:
            from .config import SDMatteConfig
            from .engine import Engine
            eng = _TRIMAP_ENGINES[index] = Engine(SDMatteConfig.tiny(), index)
        return eng


def _fan_out(model, batch):
    """Multi-GPU fan-out of one node call.  OPT-IN (SDMATTE_MULTI_GPU=1): every extra GPU receives its own copy of the packed weights
    (~12 GB in the default precision) plus an activation arena, outside ComfyUI's memory manager, and those GPUs may belong to
    other models or processes.  Used when the batch has more than one image and more than one GPU is visible; the extra engines
    live as long as the cached model they were copied from (`unload_models()` frees them)."""
    if batch < 2 or os.environ.get("SDMATTE_MULTI_GPU", "0") != "1" or not torch.cuda.is_available():
        return None
    ndev = torch.cuda.device_count()
    if ndev < 2:
        return None
    fan = getattr(model, "_fan", None)
    if fan is None:
        from .parallel import MultiGpuEngine
        first = model.engine
        fan = MultiGpuEngine.around(first, [d for d in range(ndev) if d != first.device])
        model._fan = fan
    return fan


def refine_and_compose(alpha_bhw, image, trimap, output_mode, mask_refine, trimap_constraint):
    """CPU tail of the node, same arithmetic and order as sdmatte_nodes.py:365-397."""
    out = alpha_bhw
    image_cpu, tri = image.cpu(), trimap.cpu()
    if mask_refine:
        fg = tri > trimap_constraint
        bg = tri < (1.0 - trimap_constraint)
        unknown = ~(fg | bg)
        ref = out.clone()
        ref[bg] = 0.0
        ref[fg] = torch.clamp(ref[fg] * 1.2, 0, 1)
        ref[(ref < 0.3) & unknown] = 0.0
        out = ref
    a4 = out.unsqueeze(-1)
    if output_mode == "alpha_only":
        matted = torch.zeros_like(image_cpu)
    elif output_mode == "matted_rgba":
        matted = torch.cat([image_cpu, a4], dim=-1)
    elif output_mode == "matted_rgb":
        matted = image_cpu * ((tri.unsqueeze(-1) > 0.2) & (a4 > 0.1)).float()
    else:
        matted = image_cpu * a4
    return out, matted


def _disk_reach(r):
    """hmax[dx] for dx = 0 .. r: the largest h with h^2 + dx^2 <= r^2 (integers only)."""
    import math
    return [math.isqrt(r * r - dx * dx) for dx in range(r + 1)]


def _column_distance(other):
    """Per pixel, the vertical distance to the nearest True of `other` [B,H,W] in its column (0 on a True pixel; beyond any radius if none)."""
    H = other.shape[1]
    far = 1 << 20
    ys = torch.arange(H, dtype=torch.int32).view(1, H, 1)
    above = torch.where(other, ys, torch.full_like(ys, -far)).cummax(dim=1).values
    below = -torch.where(other, -ys, torch.full_like(ys, -far - H)).flip(1).cummax(dim=1).values.flip(1)
    return torch.minimum(ys - above, below - ys)


def _near(other, r):
    """True where a True pixel of `other` lies within the closed Euclidean disk of radius r (pixels beyond the border do not exist)."""
    W = other.shape[2]
    dist = _column_distance(other)
    hit = torch.zeros_like(other)
    for dx, h in [(s * d, h) for d, h in enumerate(_disk_reach(r)) for s in ((1, -1) if d else (1,))]:
        lo, hi = max(0, -dx), W - max(0, dx)      # pixels x whose column x + dx exists
        if hi > lo:
            hit[:, :, lo:hi] |= dist[:, :, lo + dx:hi + dx] <= h
    return hit


def trimap_from_mask(mask, threshold=0.5, erode_px=10, dilate_px=10):
    """`Engine.make_trimap` on CPU tensors, bit for bit (the restatement the tests compare the kernels with): mask [B,H,W] -> fp32 trimap of
    1.0 (mask > threshold and no other pixel within erode_px), 0.0 (mask <= threshold or NaN, and no foreground within dilate_px), 0.5 elsewhere."""
    if mask.dim() != 3:
        raise ValueError(f"trimap_from_mask: mask must be [B,H,W], got {tuple(mask.shape)}")
    for name, r in (("erode_px", erode_px), ("dilate_px", dilate_px)):
        if int(r) != r or not 0 <= int(r) <= 255:
            raise ValueError(f"trimap_from_mask: {name} must be an integer in 0 .. 255, got {r!r}")
    fg = mask.detach().cpu().float() > torch.tensor(float(threshold), dtype=torch.float32)
    unknown = (fg & _near(~fg, int(erode_px))) | (~fg & _near(fg, int(dilate_px)))
    out = fg.float()
    out[unknown] = 0.5
    return out


def _component_roots(cls, conn8):
    """cls bool [H,W] -> int64 [H,W]: per pixel of the class the smallest flat index y*W + x of its component (8- or 4-connected), H*W elsewhere.
    Label equivalence in numpy: every pixel takes the smallest label around it, hooks its root to it, then all pointers are jumped to their roots;
    repeated until nothing moves.  Labels are pixel indices of the component and only decrease, so the fixed point is the component's smallest index."""
    import numpy as np
    H, W = cls.shape
    n = H * W
    flat = cls.ravel()
    lab = np.where(flat, np.arange(n, dtype=np.int64), n)
    lab = np.append(lab, n)                                   # slot n: "no pixel", its own root
    idx = np.flatnonzero(flat)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if conn8 else [])
    while True:
        grid = lab[:n].reshape(H, W)
        best = grid.copy()
        for dy, dx in steps:
            for sy, sx in ((dy, dx), (-dy, -dx)):
                y0, y1, x0, x1 = max(0, -sy), H - max(0, sy), max(0, -sx), W - max(0, sx)
                if y1 > y0 and x1 > x0:
                    np.minimum(best[y0:y1, x0:x1], grid[y0 + sy:y1 + sy, x0 + sx:x1 + sx], out=best[y0:y1, x0:x1])
        best = best.ravel()[idx]
        low = best < lab[idx]
        if not low.any():
            return lab[:n].reshape(H, W)
        np.minimum.at(lab, lab[idx][low], best[low])
        while True:
            nxt = lab[lab[idx]]
            if np.array_equal(nxt, lab[idx]):
                break
            lab[idx] = nxt


def clean_mask(mask, threshold=0.5, min_area=64, keep_largest=False, max_hole_area=64, binarize=False, return_stats=False):
    """`Engine.clean_mask` on CPU tensors, bit for bit (compares and counts only; the definition is in include/sdmatte.h, sdm_clean_mask): mask [B,H,W] ->
    fp32 [B,H,W], and with return_stats int32 [B,4] = per image {components, components removed, holes filled, pixels whose class changed}."""
    import numpy as np
    if mask.dim() != 3 or mask.numel() == 0:
        raise ValueError(f"clean_mask: mask must be a non-empty [B,H,W], got {tuple(mask.shape)}")
    thr = np.float32(threshold)
    if not (np.float32(0) <= thr < np.float32(1)) or not 0.0 <= float(threshold) < 1.0:
        raise ValueError(f"clean_mask: threshold must be in [0, 1), got {threshold!r}")
    for name, v in (("min_area", min_area), ("max_hole_area", max_hole_area)):
        if int(v) != v or not 0 <= int(v) <= (1 << 28):
            raise ValueError(f"clean_mask: {name} must be an integer in 0 .. {1 << 28}, got {v!r}")
    m = mask.detach().cpu().float().contiguous().numpy()
    B, H, W = m.shape
    n = H * W
    out = m.copy()
    stats = np.zeros((B, 4), np.int32)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            fg = m[b] > thr
        keep = fg
        if min_area > 1 or keep_largest or return_stats:
            roots = _component_roots(fg, True).ravel()
            area = np.bincount(roots, minlength=n + 1)[:n]
            ids = np.flatnonzero(area)                         # ascending = by smallest pixel index
            stats[b, 0] = ids.size
            if min_area > 1 or keep_largest:
                ok = area[ids] >= min_area
                if keep_largest and ids.size:
                    ok &= ids == ids[np.argmax(area[ids])]      # argmax: the first of equal areas
                good = np.zeros(n + 1, bool)
                good[ids[ok]] = True
                keep = good[roots].reshape(H, W)
                stats[b, 1] = int((~ok).sum())
        filled = np.zeros_like(fg)
        if max_hole_area > 0:
            roots = _component_roots(~keep, False).ravel()
            area = np.bincount(roots, minlength=n + 1)[:n]
            edge = np.zeros((H, W), bool)
            edge[0] = edge[-1] = True
            edge[:, 0] = edge[:, -1] = True
            open_ = np.zeros(n + 1, bool)
            open_[roots[edge.ravel()]] = True
            ids = np.flatnonzero(area)
            holes = ids[~open_[ids] & (area[ids] <= max_hole_area)]
            good = np.zeros(n + 1, bool)
            good[holes] = True
            filled = good[roots].reshape(H, W)
            stats[b, 2] = holes.size
        removed = fg & ~keep
        if binarize:
            out[b] = fg.astype(np.float32)
        out[b][removed] = 0.0
        out[b][filled] = 1.0
        stats[b, 3] = int(removed.sum()) + int(filled.sum())
    out = torch.from_numpy(out)
    return (out, torch.from_numpy(stats)) if return_stats else out


def subject_roi(plane, roi_threshold=0.0, margin_px=16, margin_pct=10, square=True):
    """`Engine.subject_roi` on CPU tensors, exactly (integers only; the definition is in include/sdmatte.h, sdm_subject_roi): plane [B,H,W] -> int32 [B,4]
    = per image {y0, x0, h, w}, the bounding box of `plane > roi_threshold` with its margin, clipped, optionally squared; the whole frame if empty."""
    import numpy as np
    from .engine import Engine
    if plane.dim() != 3 or plane.numel() == 0:
        raise ValueError(f"subject_roi: plane must be a non-empty [B,H,W], got {tuple(plane.shape)}")
    roi_threshold, margin_px, margin_pct = Engine._check_roi_params("subject_roi", roi_threshold, margin_px, margin_pct)
    p = plane.detach().cpu().float().contiguous().numpy()
    B, H, W = p.shape
    out = np.zeros((B, 4), np.int32)

    def axis(lo, hi, n):
        m = margin_px + ((hi - lo + 1) * margin_pct) // 100
        a = max(0, lo - m)
        return a, min(n, hi + 1 + m) - a

    def grow(a, ext, L, n):
        a -= (L - ext) // 2
        a = max(a, 0)
        if a + L > n:
            a = max(0, n - L)
        return a, min(L, n)

    for b in range(B):
        with np.errstate(invalid="ignore"):
            u = p[b] > np.float32(roi_threshold)
        rows, cols = np.flatnonzero(u.any(axis=1)), np.flatnonzero(u.any(axis=0))
        if rows.size == 0:
            out[b] = (0, 0, H, W)
            continue
        (y0, h), (x0, w) = axis(int(rows[0]), int(rows[-1]), H), axis(int(cols[0]), int(cols[-1]), W)
        if square:
            L = max(h, w)
            (y0, h), (x0, w) = grow(y0, h, L, H), grow(x0, w, L, W)
        out[b] = (y0, x0, h, w)
    return torch.from_numpy(out)


def paste_roi(crop_bhw, roi, H, W):
    """The way back of `Engine.apply_matte_roi` on CPU tensors: crop_bhw[b] ([h,w] of roi[b]; a tensor [B,h,w] or a list of planes) -> fp32 [B,H,W] that holds
    it at (y0, x0) and 0.0 everywhere else."""
    roi = torch.as_tensor(roi).reshape(-1, 4)
    if len(crop_bhw) != roi.shape[0]:
        raise ValueError(f"paste_roi: {len(crop_bhw)} crops for {roi.shape[0]} boxes")
    out = torch.zeros(roi.shape[0], int(H), int(W), dtype=torch.float32)
    for b, crop in enumerate(crop_bhw):
        y0, x0, h, w = (int(v) for v in roi[b])
        if tuple(crop.shape) != (h, w) or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
            raise ValueError(f"paste_roi: crop {tuple(crop.shape)} does not fit the box {(y0, x0, h, w)} of a {(int(H), int(W))} frame")
        out[b, y0:y0 + h, x0:x0 + w] = crop.detach().cpu().float()
    return out


def subject_boxes(plane, roi_threshold=0.0, min_area=64, max_boxes=4, margin_px=16, margin_pct=10, square=True, return_count=False):
    """`Engine.subject_boxes` on CPU tensors, exactly (integers only; the definition is in include/sdmatte.h, sdm_subject_boxes): plane [B,H,W] -> int32
    [B,max_boxes,5] = per image the entries {b, y0, x0, h, w}, void entries {-1, 0, 0, 0, 0} behind them; with return_count also int32 [B]."""
    import numpy as np
    from .engine import Engine
    if plane.dim() != 3 or plane.numel() == 0:
        raise ValueError(f"subject_boxes: plane must be a non-empty [B,H,W], got {tuple(plane.shape)}")
    roi_threshold, margin_px, margin_pct = Engine._check_roi_params("subject_boxes", roi_threshold, margin_px, margin_pct)
    min_area, max_boxes = Engine._check_boxes_params("subject_boxes", min_area, max_boxes)
    p = plane.detach().cpu().float().contiguous().numpy()
    B, H, W = p.shape
    n = H * W
    out = np.zeros((B, max_boxes, 5), np.int32)
    out[:, :, 0] = -1
    count = np.zeros(B, np.int32)

    def box_of(u):
        """subject_roi's rule on the extrema of the non-empty set u (bool [H,W])."""
        return [int(v) for v in subject_roi(torch.from_numpy(u[None].astype(np.float32)), 0.0, margin_px, margin_pct, square)[0]]

    for b in range(B):
        with np.errstate(invalid="ignore"):
            u = p[b] > np.float32(roi_threshold)
        entries = []
        if u.any():
            roots = _component_roots(u, True)
            area = np.bincount(roots.ravel(), minlength=n + 1)[:n]
            ids = np.flatnonzero(area)
            ids = ids[area[ids] >= min_area]
            order = ids[np.argsort(-area[ids], kind="stable")][:max_boxes - 1]      # stable: equal areas stay in root order
            covered = np.zeros((H, W), bool)
            for r in order:
                comp = roots == r
                rows, cols = np.flatnonzero(comp.any(axis=1)), np.flatnonzero(comp.any(axis=0))
                if any(y0 <= rows[0] and rows[-1] < y0 + h and x0 <= cols[0] and cols[-1] < x0 + w for y0, x0, h, w in entries):
                    continue
                y0, x0, h, w = box_of(comp)
                entries.append((y0, x0, h, w))
                covered[y0:y0 + h, x0:x0 + w] = True
            rest = u & ~covered
            if rest.any():
                entries.append(tuple(box_of(rest)))
        else:
            entries.append((0, 0, H, W))
        for i, e in enumerate(entries):
            out[b, i] = (b, ) + tuple(e)
        count[b] = len(entries)
    out = torch.from_numpy(out)
    return (out, torch.from_numpy(count)) if return_count else out


def compact_boxes(boxes):
    """The entries of a box list (int [..,5] = {b, y0, x0, h, w}) that are not void (b >= 0), in their order, as int32 [N,5] on the host."""
    flat = torch.as_tensor(boxes).detach().cpu().reshape(-1, 5).to(torch.int32)
    return flat[flat[:, 0] >= 0].contiguous()


def paste_boxes(crops, boxes, B, H, W):
    """The way back of `Engine.apply_matte_boxes` on CPU tensors: crops[n] ([h,w] of boxes[n] = {b, y0, x0, h, w}) -> fp32 [B,H,W], each crop pasted into
    zeros at (y0, x0) of image b, the element-wise maximum where several meet.  A void entry (b < 0) is skipped."""
    boxes = torch.as_tensor(boxes).reshape(-1, 5)
    if len(crops) != boxes.shape[0]:
        raise ValueError(f"paste_boxes: {len(crops)} crops for {boxes.shape[0]} boxes")
    out = torch.zeros(int(B), int(H), int(W), dtype=torch.float32)
    for n, crop in enumerate(crops):
        b, y0, x0, h, w = (int(v) for v in boxes[n])
        if b < 0:
            continue
        if b >= B or tuple(crop.shape) != (h, w) or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
            raise ValueError(f"paste_boxes: crop {tuple(crop.shape)} does not fit the box {(b, y0, x0, h, w)} of {int(B)} frames of {(int(H), int(W))}")
        out[b] = torch.maximum(out[b], paste_roi(crop[None], [[y0, x0, h, w]], H, W)[0])
    return out


def tile_axis(L, tile, overlap):
    """The grid rule of `Engine.band_tiles` for one axis of length L, in Python integers (the definition is in include/sdmatte.h, sdm_band_tiles):
    (origins, size) - one tile of size L at 0 if L <= tile, otherwise n = ceil((L - overlap) / (tile - overlap)) tiles of size `tile` at
    (i * (L - tile)) // (n - 1)."""
    L, tile, overlap = int(L), int(tile), int(overlap)
    if L < 1 or tile < 1 or not 0 <= overlap <= tile // 2:
        raise ValueError(f"tile_axis: L = {L}, tile = {tile}, overlap = {overlap}: need L >= 1, tile >= 1 and overlap in 0 .. tile / 2")
    if L <= tile:
        return [0], L
    n = -(-(L - overlap) // (tile - overlap))
    return [(i * (L - tile)) // (n - 1) for i in range(n)], tile


def band_tiles(trimap, band_lo=0.25, band_hi=0.75, tile=1024, overlap=128, max_tiles=16, return_count=False):
    """`Engine.band_tiles` on CPU tensors, exactly (integers only): trimap [B,H,W] -> int32 [B,max_tiles,5] = per image the entries {b, y0, x0, h, w} of
    the grid tiles that hold a pixel with band_lo < trimap < band_hi (compared in fp32), row-major, void entries {-1, 0, 0, 0, 0} behind them; with
    return_count also int32 [B], the number of such tiles (also beyond max_tiles).  A tile's band pixels are counted through a summed-area table."""
    import numpy as np
    from .engine import Engine
    if trimap.dim() != 3 or trimap.numel() == 0:
        raise ValueError(f"band_tiles: trimap must be a non-empty [B,H,W], got {tuple(trimap.shape)}")
    band_lo, band_hi, tile, overlap, max_tiles = Engine._check_tiles_params("band_tiles", band_lo, band_hi, tile, overlap, max_tiles)
    p = trimap.detach().cpu().float().contiguous().numpy()
    B, H, W = p.shape
    Engine._check_tiles_grid("band_tiles", H, W, tile, overlap)
    (oy, sy), (ox, sx) = tile_axis(H, tile, overlap), tile_axis(W, tile, overlap)
    out = np.zeros((B, max_tiles, 5), np.int32)
    out[:, :, 0] = -1
    count = np.zeros(B, np.int32)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            band = (p[b] > np.float32(band_lo)) & (p[b] < np.float32(band_hi))
        sat = np.zeros((H + 1, W + 1), np.int64)
        sat[1:, 1:] = band.astype(np.int64).cumsum(0).cumsum(1)
        n = 0
        for y0 in oy:
            for x0 in ox:
                if sat[y0 + sy, x0 + sx] - sat[y0, x0 + sx] - sat[y0 + sy, x0] + sat[y0, x0] > 0:
                    if n < max_tiles:
                        out[b, n] = (b, y0, x0, sy, sx)
                    n += 1
        count[b] = n
    out = torch.from_numpy(out)
    return (out, torch.from_numpy(count)) if return_count else out


def _tile_axis_weight(start, ext, L, feather_px):
    """fp32 [ext]: min(1, (d + 1) / (feather_px + 1)) with d the distance to the nearer edge pixel among the tile's sides that are not on the frame's
    border (1.0 without such a side)."""
    o = torch.arange(ext, dtype=torch.int64)
    d = torch.full((ext, ), 1 << 40, dtype=torch.int64)
    if start != 0:
        d = torch.minimum(d, o)
    if start + ext != L:
        d = torch.minimum(d, ext - 1 - o)
    ramp = (d.clamp(max=feather_px) + 1).to(torch.float32) / torch.tensor(float(feather_px + 1), dtype=torch.float32)
    return torch.where(d >= feather_px, torch.ones(ext, dtype=torch.float32), ramp)


def blend_tiles(crops, tiles, B, H, W, feather_px=0, base=None):
    """The way back of `Engine.apply_matte_tiles` on CPU tensors, in fp32 and in list order (the definition is in include/sdmatte.h,
    sdm_apply_matte_tiles): crops[n] ([h,w] of tiles[n] = {b, y0, x0, h, w}, values in [0, 1]) -> fp32 [B,H,W], per pixel
    clamp(sum (w_n / Wsum) * crops[n]) over the tiles that contain it, w_n = wy * wx ramping over feather_px pixels towards a tile's edges inside the
    frame; a pixel in no tile gets `base` [B,H,W] (NaN -> 0, clamped; None: 0.0).  A void entry (b < 0) is skipped."""
    tiles = torch.as_tensor(tiles).reshape(-1, 5)
    B, H, W, feather_px = int(B), int(H), int(W), int(feather_px)
    if len(crops) != tiles.shape[0]:
        raise ValueError(f"blend_tiles: {len(crops)} crops for {tiles.shape[0]} tiles")
    if feather_px < 0:
        raise ValueError(f"blend_tiles: feather_px must be >= 0, got {feather_px}")
    if base is None:
        out = torch.zeros(B, H, W, dtype=torch.float32)
    else:
        if tuple(base.shape) != (B, H, W):
            raise ValueError(f"blend_tiles: base must be [B,H,W] = {(B, H, W)}, got {tuple(base.shape)}")
        out = torch.nan_to_num(base.detach().cpu().float(), nan=0.0).clamp(0.0, 1.0)
    wsum = torch.zeros(B, H, W, dtype=torch.float32)
    acc = torch.zeros(B, H, W, dtype=torch.float32)
    weights = []
    for n, crop in enumerate(crops):
        b, y0, x0, h, w = (int(v) for v in tiles[n])
        if b < 0:
            weights.append(None)
            continue
        if b >= B or tuple(crop.shape) != (h, w) or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
            raise ValueError(f"blend_tiles: crop {tuple(crop.shape)} does not fit the tile {(b, y0, x0, h, w)} of {B} frames of {(H, W)}")
        wn = _tile_axis_weight(y0, h, H, feather_px)[:, None] * _tile_axis_weight(x0, w, W, feather_px)[None, :]
        weights.append(wn)
        wsum[b, y0:y0 + h, x0:x0 + w] += wn
    for n, crop in enumerate(crops):
        if weights[n] is None:
            continue
        b, y0, x0, h, w = (int(v) for v in tiles[n])
        acc[b, y0:y0 + h, x0:x0 + w] += (weights[n] / wsum[b, y0:y0 + h, x0:x0 + w]) * crop.detach().cpu().float()
    covered = wsum > 0
    out[covered] = acc.clamp(0.0, 1.0)[covered]
    return out


def auto_tile(H, W, inference_size, overlap=128, limit=16):
    """The tile size of the tiled node: the smallest multiple of 64 that is >= inference_size and whose grid (the rule of `tile_axis`) has at most `limit`
    cells on an H x W frame.  No data is read, so the result bounds the tile count of every image of that size."""
    H, W, overlap, limit = int(H), int(W), int(overlap), int(limit)
    if H < 1 or W < 1 or limit < 1 or int(inference_size) < 1 or overlap < 0:
        raise ValueError(f"auto_tile: bad arguments H = {H}, W = {W}, inference_size = {inference_size}, overlap = {overlap}, limit = {limit}")
    tile = -(-int(inference_size) // 64) * 64
    while tile // 2 < overlap or len(tile_axis(H, tile, overlap)[0]) * len(tile_axis(W, tile, overlap)[0]) > limit:
        tile += 64
    return tile


def canvas_fit(roi, canvas_h, canvas_w, fill_pct=80, valign="center"):
    """The placements of `Engine.compose_canvas` in exact integers (the definition is in include/sdmatte.h, sdm_compose_canvas): roi int [B,4] = {y0, x0, h, w}
    -> int32 [B,8] = {y0, x0, h, w, dy0, dx0, dh, dw}, the box scaled to fill `fill_pct` % of the canvas and aligned in it."""
    from .engine import Engine
    canvas_h, canvas_w, fill_pct, valign, *_ = Engine._check_canvas_params("canvas_fit", 1, canvas_h, canvas_w, fill_pct, valign, 0.0, 1.0, 0, 0)
    roi = torch.as_tensor(roi).reshape(-1, 4)
    th, tw = max(1, canvas_h * fill_pct // 100), max(1, canvas_w * fill_pct // 100)
    mv = (canvas_h - th) // 2
    out = []
    for y0, x0, h, w in roi.tolist():
        if h < 1 or w < 1:
            raise ValueError(f"canvas_fit: empty box {(y0, x0, h, w)}")
        if th * w <= tw * h:
            dh, dw = th, max(1, (w * th + h // 2) // h)
        else:
            dw, dh = tw, max(1, (h * tw + w // 2) // w)
        dy0 = (mv, (canvas_h - dh) // 2, canvas_h - mv - dh)[valign]
        out.append((y0, x0, h, w, dy0, (canvas_w - dw) // 2, dh, dw))
    return torch.tensor(out, dtype=torch.int32).reshape(-1, 8)


def _shadow_weights(shadow_sigma):
    """(r, the 2r + 1 weights of offsets -r .. r as float32 values): exp(-i^2 / (2 sigma^2)) / sum in double from the fp32 sigma."""
    import math
    import numpy as np
    s = float(np.float32(shadow_sigma))
    r = max(1, math.ceil(3.0 * s))
    g = [math.exp(-(i * i) / (2.0 * s * s)) for i in range(-r, r + 1)]
    total = 0.0
    for v in g:
        total += v
    return r, [float(np.float32(v / total)) for v in g]


def compose_canvas(fg, alpha, canvas_h, canvas_w, fill_pct=80, valign="center", bg_color=None, bg_image=None, shadow_opacity=0.0, shadow_sigma=8.0,
                   shadow_dy=0, shadow_dx=0, roi_threshold=0.0, out_channels=None, dtype=torch.float32, return_placement=False):
    """`Engine.compose_canvas` in torch (the definition is in include/sdmatte.h, sdm_compose_canvas), evaluated in `dtype` (float32: equal to the GPU call up to
    fp32 rounding; float64: the reference the tests measure both against).  Built on `subject_roi`, `canvas_fit` and
    torch.nn.functional.interpolate(mode="bilinear", antialias=True) of the premultiplied box.  Runs on the device of `fg`."""
    import torch.nn.functional as F
    from .engine import Engine
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"compose_canvas: dtype must be torch.float32 or torch.float64, got {dtype!r}")
    if fg.dim() != 4 or fg.shape[-1] != 3 or fg.numel() == 0:
        raise ValueError(f"compose_canvas: fg must be a non-empty [B,H,W,3], got {tuple(fg.shape)}")
    B, H, W, _ = (int(v) for v in fg.shape)
    if tuple(alpha.shape) != (B, H, W):
        raise ValueError(f"compose_canvas: alpha must be [B,H,W] = {(B, H, W)}, got {tuple(alpha.shape)}")
    canvas_h, canvas_w, fill_pct, valign, shadow_opacity, shadow_sigma, shadow_dy, shadow_dx = Engine._check_canvas_params(
        "compose_canvas", B, canvas_h, canvas_w, fill_pct, valign, shadow_opacity, shadow_sigma, shadow_dy, shadow_dx)
    bg_mode = 2 if bg_image is not None else (1 if bg_color is not None else 0)
    if out_channels is None:
        out_channels = 3 if bg_mode else 4
    if out_channels not in (3, 4) or (bg_mode == 0 and out_channels != 4):
        raise ValueError(f"compose_canvas: out_channels must be 4, or 3 with a background, got {out_channels!r}")
    dev = fg.device
    alpha = alpha.detach().float()
    place = canvas_fit(subject_roi(alpha, roi_threshold, 0, 0, False), canvas_h, canvas_w, fill_pct, valign)
    a = torch.nan_to_num(alpha.to(dtype), nan=0.0).clamp(0.0, 1.0)
    prem = torch.cat([a.unsqueeze(1) * fg.detach().float().to(dtype).permute(0, 3, 1, 2), a.unsqueeze(1)], 1)          # [B,4,H,W] = (a F, a)
    layer = torch.zeros(B, 4, canvas_h, canvas_w, dtype=dtype, device=dev)
    for b, (y0, x0, h, w, dy0, dx0, dh, dw) in enumerate(place.tolist()):
        crop = prem[b:b + 1, :, y0:y0 + h, x0:x0 + w]
        if (dh, dw) != (h, w):
            crop = F.interpolate(crop, size=(dh, dw), mode="bilinear", align_corners=False, antialias=True)
        layer[b, :, dy0:dy0 + dh, dx0:dx0 + dw] = crop[0]
    Ps, As = layer[:, :3], layer[:, 3:]
    S = torch.zeros_like(As)
    if shadow_opacity > 0.0:
        r, wts = _shadow_weights(shadow_sigma)
        px, py = r + abs(shadow_dx), r + abs(shadow_dy)
        src = F.pad(As, (px, px, 0, 0))
        T = torch.zeros_like(As)
        for k, wk in enumerate(wts):                        # rows first, i ascending
            o = px - shadow_dx + k - r
            T = T + wk * src[..., o:o + canvas_w]
        src = F.pad(T, (0, 0, py, py))
        for k, wk in enumerate(wts):
            o = py - shadow_dy + k - r
            S = S + wk * src[:, :, o:o + canvas_h, :]
        S = shadow_opacity * S
    if bg_mode == 2:
        if bg_image.dim() != 4 or tuple(bg_image.shape[1:]) != (canvas_h, canvas_w, 3) or int(bg_image.shape[0]) not in (1, B):
            raise ValueError(f"compose_canvas: bg_image must be [1 or {B},{canvas_h},{canvas_w},3], got {tuple(bg_image.shape)}")
        C = bg_image.detach().float().to(dtype).to(dev).permute(0, 3, 1, 2)
    elif bg_mode == 1:
        rgb = [float(v) for v in bg_color]
        if len(rgb) != 3:
            raise ValueError(f"compose_canvas: bg_color must be 3 numbers, got {bg_color!r}")
        C = torch.tensor(rgb, dtype=torch.float32, device=dev).to(dtype).reshape(1, 3, 1, 1)
    else:
        C = torch.zeros(1, 3, 1, 1, dtype=dtype, device=dev)
    P = Ps + (1.0 - As) * ((1.0 - S) * C)
    A = torch.ones_like(As) if bg_mode else As + (1.0 - As) * S
    if out_channels == 4:
        P = torch.cat([torch.where(A > 0, P / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(P)), A], 1)
    out = P.permute(0, 2, 3, 1).contiguous()
    return (out, place) if return_placement else out


def _nearest_index(n_dst, n_src):
    """src = min(n_src - 1, (i * n_src) // n_dst) for i = 0 .. n_dst - 1 (integers only)."""
    return torch.clamp((torch.arange(n_dst, dtype=torch.int64) * n_src) // n_dst, max=n_src - 1)


def _neighbours(t):
    """t [B,h,w,...] -> its left, right, up and down neighbours, coordinates clamped to the level (a border pixel is its own neighbour)."""
    return (torch.cat([t[:, :, :1], t[:, :, :-1]], 2), torch.cat([t[:, :, 1:], t[:, :, -1:]], 2),
            torch.cat([t[:, :1], t[:, :-1]], 1), torch.cat([t[:, 1:], t[:, -1:]], 1))


def estimate_foreground(image, alpha, regularization=1e-5, gradient_weight=1.0, n_small_iters=10, n_big_iters=2):
    """`Engine.estimate_foreground` on CPU tensors in fp32 (the multi-level estimator defined in include/sdmatte.h): image [B,H,W,3], alpha [B,H,W] ->
    (fg [B,H,W,3], bg [B,H,W,3], sanitised alpha [B,H,W]).  It and the GPU kernels evaluate the same formulas in fp32 but not in the same order
    (summation order, FMA contraction), so they agree to rounding, not bit for bit."""
    from .engine import Engine
    if image.dim() != 4 or image.shape[-1] != 3 or image.numel() == 0:
        raise ValueError(f"estimate_foreground: image must be a non-empty [B,H,W,3], got {tuple(image.shape)}")
    if tuple(alpha.shape) != tuple(image.shape[:3]):
        raise ValueError(f"estimate_foreground: alpha must be [B,H,W] = {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
    reg, gw, n_small, n_big = Engine._check_fg_params("estimate_foreground", regularization, gradient_weight, n_small_iters, n_big_iters)
    image = image.detach().cpu().float()
    alpha = torch.nan_to_num(alpha.detach().cpu().float(), nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)
    H, W = int(image.shape[1]), int(image.shape[2])
    sizes = [(H, W)]
    while sizes[-1] != (1, 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    F = B = None
    for h, w in reversed(sizes):
        iy, ix = _nearest_index(h, H), _nearest_index(w, W)
        I = image[:, iy][:, :, ix]
        a0 = alpha[:, iy][:, :, ix].unsqueeze(-1)
        if F is None:
            F, B = I.clone(), I.clone()
        else:
            py, px = _nearest_index(h, F.shape[1]), _nearest_index(w, F.shape[2])
            F, B = F[:, py][:, :, px], B[:, py][:, :, px]
        a1 = 1.0 - a0
        wq = [reg + gw * (a0 - q).abs() for q in _neighbours(a0)]
        s = wq[0] + wq[1] + wq[2] + wq[3]
        D = a0 * a0 + a1 * a1 + s
        for _ in range(n_small if max(h, w) <= 32 else n_big):
            Fq, Bq = _neighbours(F), _neighbours(B)
            Fm = (wq[0] * Fq[0] + wq[1] * Fq[1] + wq[2] * Fq[2] + wq[3] * Fq[3]) / s
            Bm = (wq[0] * Bq[0] + wq[1] * Bq[1] + wq[2] * Bq[2] + wq[3] * Bq[3]) / s
            r = (I - a0 * Fm - a1 * Bm) / D
            F, B = (Fm + a0 * r).clamp(0.0, 1.0), (Bm + a1 * r).clamp(0.0, 1.0)
    return F.contiguous(), B.contiguous(), alpha


def auto_subsample(H, W, inference_size):
    """The factor between an (H, W) image and the resolution the model saw it at: clamp(ceil(max(H, W) / inference_size), 1, 16)."""
    H, W, inference_size = int(H), int(W), int(inference_size)
    if H < 1 or W < 1 or inference_size < 1:
        raise ValueError(f"auto_subsample: sizes must be positive, got {(H, W, inference_size)}")
    return min(max(-(-max(H, W) // inference_size), 1), 16)


def _window_mean(t, radius):
    """Mean of t [B,h,w,C] over the (2 radius + 1)^2 window clipped to the grid: direct sums along x, then along y, divided by the window's count."""
    for axis in (2, 1):
        n = t.shape[axis]
        acc = torch.zeros_like(t)
        for d in range(-radius, radius + 1):
            lo, hi = max(0, -d), n - max(0, d)          # entries i whose neighbour i + d exists
            if hi > lo:
                acc.narrow(axis, lo, hi - lo).add_(t.narrow(axis, lo + d, hi - lo))
        t = acc
    h, w = t.shape[1], t.shape[2]
    iy, ix = torch.arange(h, device=t.device), torch.arange(w, device=t.device)
    ny = torch.clamp(iy + radius, max=h - 1) - torch.clamp(iy - radius, min=0) + 1
    nx = torch.clamp(ix + radius, max=w - 1) - torch.clamp(ix - radius, min=0) + 1
    return t / (ny[:, None] * nx[None, :]).to(t.dtype)[None, :, :, None]


def _bilinear_axis(n_full, n_coarse, s, device):
    u = ((torch.arange(n_full, dtype=torch.float32, device=device) + 0.5) / float(s) - 0.5).clamp(0.0, float(n_coarse - 1))
    i0 = u.floor().long()
    return i0, torch.clamp(i0 + 1, max=n_coarse - 1), u - i0.float()


def guided_refine_alpha(image, alpha, subsample, radius=2, eps=1e-4):
    """`Engine.refine_alpha_guided` in torch fp32, on the tensors' own device (the subsampled colour guided filter defined in include/sdmatte.h):
    image [B,H,W,3], alpha [B,H,W] -> refined alpha [B,H,W] in [0,1].  It and the GPU kernels evaluate the same formulas in fp32 but not in the same
    order (summation order, FMA contraction), so they agree to rounding, not bit for bit."""
    from .engine import Engine
    import torch.nn.functional as F
    if image.dim() != 4 or image.shape[-1] != 3 or image.numel() == 0:
        raise ValueError(f"guided_refine_alpha: image must be a non-empty [B,H,W,3], got {tuple(image.shape)}")
    if tuple(alpha.shape) != tuple(image.shape[:3]):
        raise ValueError(f"guided_refine_alpha: alpha must be [B,H,W] = {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
    s, radius, eps = Engine._check_gf_params("guided_refine_alpha", subsample, radius, eps)
    image = image.detach().float()
    p = torch.nan_to_num(alpha.detach().float(), nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)
    B, H, W = p.shape
    h, w = -(-H // s), -(-W // s)
    x = torch.cat([image, p.unsqueeze(-1)], -1)
    # block means over the existing pixels: zero-pad to whole blocks, sum, divide by the count
    x = F.pad(x, (0, 0, 0, w * s - W, 0, h * s - H)).view(B, h, s, w, s, 4).sum(dim=(2, 4))
    cy = torch.clamp(torch.arange(h, device=x.device) * s + s, max=H) - torch.arange(h, device=x.device) * s
    cx = torch.clamp(torch.arange(w, device=x.device) * s + s, max=W) - torch.arange(w, device=x.device) * s
    x = x / (cy[:, None] * cx[None, :]).float()[None, :, :, None]
    Ic, pc = x[..., :3], x[..., 3:]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    m = _window_mean(torch.cat([Ic, pc, Ic * pc] + [Ic[..., i:i + 1] * Ic[..., j:j + 1] for i, j in pairs], -1), radius)       # the 13 moments
    mu, mup = m[..., 0:3], m[..., 3]
    c = m[..., 4:7] - mu * mup.unsqueeze(-1)
    s00, s01, s02, s11, s12, s22 = (m[..., 7 + k] - mu[..., i] * mu[..., j] + (eps if i == j else 0.0) for k, (i, j) in enumerate(pairs))
    k00, k01, k02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
    k11, k12, k22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
    det = s00 * k00 + s01 * k01 + s02 * k02
    a = torch.stack([k00 * c[..., 0] + k01 * c[..., 1] + k02 * c[..., 2], k01 * c[..., 0] + k11 * c[..., 1] + k12 * c[..., 2],
                     k02 * c[..., 0] + k12 * c[..., 1] + k22 * c[..., 2]], -1) / det.unsqueeze(-1)
    b = mup - (a * mu).sum(-1)
    ab = _window_mean(torch.cat([a, b.unsqueeze(-1)], -1), radius)
    i0, i1, fy = _bilinear_axis(H, h, s, ab.device)
    j0, j1, fx = _bilinear_axis(W, w, s, ab.device)
    rows = (1.0 - fy)[None, :, None, None] * ab[:, i0] + fy[None, :, None, None] * ab[:, i1]
    up = (1.0 - fx)[None, None, :, None] * rows[:, :, j0] + fx[None, None, :, None] * rows[:, :, j1]
    return ((up[..., :3] * image).sum(-1) + up[..., 3]).clamp(0.0, 1.0).contiguous()


DF_NONE = 2147483647      # SDM_DF_NONE (include/sdmatte.h)
OUTLINE_POSITION = {"outside": 0, "center": 1, "inside": 2}


def _nearest_other_sq(other):
    """other: bool [H,W].  int64 [H,W]: the squared distance of every pixel to the nearest True pixel, DF_NONE without one.  Exact: column distances by
    two running scans, then the lower envelope of the rows' parabolas by an outward search that stops once dx^2 reaches the largest best."""
    import numpy as np
    H, W = other.shape
    big = np.int64(1) << 40
    if not other.any():
        return np.full((H, W), DF_NONE, np.int64)
    rows = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(other, rows, -big), axis=0)                      # row of the nearest True pixel at or above
    below = np.minimum.accumulate(np.where(other, rows, big)[::-1], axis=0)[::-1]           # ... at or below
    g = np.minimum(rows - above, below - rows)
    g2 = np.where(g >= big // 2, big, g * g)
    best = g2.copy()
    for dx in range(1, W):
        d2 = np.int64(dx) * dx
        if d2 >= best.max():
            break
        np.minimum(best[:, dx:], g2[:, :-dx] + d2, out=best[:, dx:])
        np.minimum(best[:, :-dx], g2[:, dx:] + d2, out=best[:, :-dx])
    return best


def distance_field(plane, threshold=0.5):
    """CPU restatement of the GPU op `Engine.distance_field` (sdm_distance_field, defined in include/sdmatte.h): plane [B,H,W] -> int32 [B,H,W], +d2 on
    the pixels of `plane > threshold`, -d2 on the others, d2 the squared Euclidean distance to the nearest pixel of the other class of the same image
    (DF_NONE where that class is empty).  Integers only: exact."""
    if plane.dim() != 3 or plane.numel() == 0:
        raise ValueError(f"distance_field: plane must be a non-empty [B,H,W], got {tuple(plane.shape)}")
    import numpy as np
    with np.errstate(invalid="ignore"):
        fg = plane.detach().cpu().float().numpy() > np.float32(threshold)
    out = np.empty(fg.shape, np.int32)
    for b in range(fg.shape[0]):
        out[b] = np.where(fg[b], _nearest_other_sq(~fg[b]), -_nearest_other_sq(fg[b])).astype(np.int32)
    return torch.from_numpy(out)


def _signed_distance(field, dtype):
    r = field.abs().to(dtype).sqrt() - 0.5
    return torch.where(field > 0, -r, r)


def _ramp(num, den):
    return (num / den + 0.5).clamp(0.0, 1.0)


def offset_mask(mask, offset_px=0.0, feather_px=1.0, threshold=0.5, dtype=torch.float32):
    """CPU restatement of the GPU op `Engine.offset_mask` (sdm_offset_mask): clamp((offset_px - sd) / feather_px + 0.5, 0, 1) with sd the signed
    distance to the silhouette of `mask > threshold`.  The parameters are rounded to fp32 first, as they cross the C ABI that way; `dtype` is the
    precision of the arithmetic (float64: the yardstick of the tests)."""
    from .engine import Engine
    Engine._check_df_plane("offset_mask", mask, threshold)
    offset_px = Engine._check_f32_range("offset_mask", "offset_px", offset_px, -Engine.DF_MAX_OFFSET, Engine.DF_MAX_OFFSET)
    feather_px = Engine._check_f32_range("offset_mask", "feather_px", feather_px, 1, Engine.DF_MAX_FEATHER)
    sd = _signed_distance(distance_field(mask, threshold), dtype)
    return _ramp(torch.tensor(offset_px, dtype=dtype) - sd, torch.tensor(feather_px, dtype=dtype))


def outline_cutout(fg, alpha, width_px=8.0, color=(1.0, 1.0, 1.0), position="outside", softness_px=1.0, opacity=1.0, edge_threshold=0.5,
                   dtype=torch.float32):
    """CPU restatement of the GPU op `Engine.outline` (sdm_outline, defined in include/sdmatte.h): (rgb [B,H,W,3], alpha [B,H,W]) of the straight-alpha
    cut-out with a stroke along the silhouette of `alpha > edge_threshold`.  Parameters rounded to fp32 first; `dtype` as in offset_mask."""
    from .engine import Engine
    if fg.dim() != 4 or fg.shape[-1] != 3 or tuple(alpha.shape) != tuple(fg.shape[:3]):
        raise ValueError(f"outline_cutout: fg must be [B,H,W,3] and alpha [B,H,W], got {tuple(fg.shape)} and {tuple(alpha.shape)}")
    Engine._check_df_plane("outline_cutout", alpha, edge_threshold)
    position = OUTLINE_POSITION.get(position, position)
    if isinstance(position, str) or int(position) != position or not 0 <= int(position) <= 2:
        raise ValueError(f"outline_cutout: position must be one of {sorted(OUTLINE_POSITION)} or 0 .. 2, got {position!r}")
    width = torch.tensor(Engine._check_f32_range("outline_cutout", "width_px", width_px, 0, Engine.OUTLINE_MAX_WIDTH, lo_open=True), dtype=torch.float32)
    soft = torch.tensor(Engine._check_f32_range("outline_cutout", "softness_px", softness_px, 1, Engine.DF_MAX_FEATHER), dtype=dtype)
    opacity = torch.tensor(Engine._check_f32_range("outline_cutout", "opacity", opacity, 0, 1), dtype=dtype)
    rgb = torch.tensor([float(v) for v in color], dtype=torch.float32)
    if rgb.shape != (3, ) or not bool(torch.isfinite(rgb).all()):
        raise ValueError(f"outline_cutout: color must be 3 finite numbers, got {color!r}")
    rgb = rgb.to(dtype)
    alpha = alpha.detach().cpu().float()
    F = fg.detach().cpu().float().to(dtype)
    sd = _signed_distance(distance_field(alpha, edge_threshold), dtype)
    # the band's edges are fp32 values (width / 2 is exact)
    hi = (width if position == 0 else (width * 0.5 if position == 1 else torch.zeros(()))).to(dtype)
    lo = (-width * 0.5 if position == 1 else -width).to(dtype)
    c = _ramp(hi - sd, soft)
    if position != 0:
        c = c * _ramp(sd - lo, soft)
    a = torch.nan_to_num(alpha, nan=0.0).clamp(0.0, 1.0).to(dtype)
    a_s = c * opacity
    ws = a_s * (1.0 - a) if position == 0 else a_s
    A = a + ws if position == 0 else a_s + a * (1.0 - a_s)
    t = torch.where(A > 0, ws / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A)).unsqueeze(-1)
    mixed = torch.where((a > 0).unsqueeze(-1), F + (rgb - F) * t, rgb.expand_as(F))
    return torch.where((A > 0).unsqueeze(-1), mixed, torch.zeros_like(F)), A


def temporal_smooth_alpha(image, alpha, radius=2, patch=1, color_tolerance=0.1, strength=1.0, max_change=1.0, clip_len=0):
    """`Engine.smooth_alpha_temporal` in torch fp32, on the tensors' own device (the image-guided temporal filter defined in include/sdmatte.h): the
    alpha [B,H,W] of B consecutive frames [B,H,W,3] -> fp32 [B,H,W] in [0,1].  Equal to the kernel to fp32 rounding, not bit for bit; the identities of
    the header (strength 0, max_change 0, one frame, clip_len 1, a hard cut, clips = separate calls) hold exactly here too.  It materialises two
    full-size tensors per offset k, which is what the kernel is there to avoid."""
    import torch.nn.functional as F
    from .engine import Engine
    if image.dim() != 4 or image.shape[-1] != 3 or image.numel() == 0:
        raise ValueError(f"temporal_smooth_alpha: image must be a non-empty [B,H,W,3], got {tuple(image.shape)}")
    if tuple(alpha.shape) != tuple(image.shape[:3]):
        raise ValueError(f"temporal_smooth_alpha: alpha must be [B,H,W] = {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
    B = int(image.shape[0])
    radius, patch, color_tolerance, strength, max_change, clip_len = Engine._check_ts_params(
        "temporal_smooth_alpha", B, radius, patch, color_tolerance, strength, max_change, clip_len)
    dev = image.device
    img = image.detach().float()
    a = torch.nan_to_num(alpha.detach().float(), nan=0.0).clamp(0.0, 1.0)
    tol = torch.tensor(color_tolerance, dtype=torch.float32, device=dev)
    tau2 = tol * tol
    clip = torch.arange(B, device=dev) // (clip_len if clip_len else B)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    num, den = a.clone(), torch.ones_like(a)
    for k in range(1, min(radius, B - 1) + 1):
        d = img[k:] - img[:-k]
        e = (d * d).sum(-1)
        if patch:          # the mean over the pixels of the patch that exist
            e = F.avg_pool2d(e.unsqueeze(1), 2 * patch + 1, 1, patch, count_include_pad=False).squeeze(1)
        u = 1.0 - (e / 3.0) / tau2
        u = torch.where(u > 0, u, zero)
        ck = torch.tensor(strength, dtype=torch.float32, device=dev) * (1.0 - torch.tensor(float(k), device=dev) / float(radius + 1))
        w = torch.where((clip[k:] == clip[:-k]).view(-1, 1, 1), ck * (u * u), zero)
        num[:-k] += w * a[k:]
        den[:-k] += w
        num[k:] += w * a[:-k]
        den[k:] += w
    limit = torch.tensor(max_change, dtype=torch.float32, device=dev)
    return (a + torch.minimum(torch.maximum(num / den - a, -limit), limit)).clamp(0.0, 1.0)


def temporal_smooth_alpha_motion(image, alpha, radius=2, patch=1, search=4, color_tolerance=0.1, motion_penalty=0.02, strength=1.0, max_change=1.0,
                                 clip_len=0):
    """`Engine.smooth_alpha_motion` in torch fp32, on the tensors' own device (the block-matched temporal filter defined in include/sdmatte.h): the alpha
    [B,H,W] of B consecutive frames [B,H,W,3] -> fp32 [B,H,W] in [0,1].  Equal to the kernel to fp32 rounding wherever the best two candidates are not
    within rounding of each other; the identities of the header hold exactly here too.  search = 0 is `temporal_smooth_alpha`.  One pass over padded
    tensors per offset k and displacement d, the candidates in the order of the choice rule (dy^2 + dx^2, dy, dx), so 'strictly smaller cost' keeps
    the lexicographic minimum."""
    import torch.nn.functional as F
    from .engine import Engine
    if image.dim() != 4 or image.shape[-1] != 3 or image.numel() == 0:
        raise ValueError(f"temporal_smooth_alpha_motion: image must be a non-empty [B,H,W,3], got {tuple(image.shape)}")
    if tuple(alpha.shape) != tuple(image.shape[:3]):
        raise ValueError(f"temporal_smooth_alpha_motion: alpha must be [B,H,W] = {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
    B, H, W = (int(v) for v in image.shape[:3])
    radius, patch, search, color_tolerance, motion_penalty, strength, max_change, clip_len = Engine._check_tsm_params(
        "temporal_smooth_alpha_motion", B, radius, patch, search, color_tolerance, motion_penalty, strength, max_change, clip_len)
    if search == 0:
        return temporal_smooth_alpha(image, alpha, radius, patch, color_tolerance, strength, max_change, clip_len)
    dev = image.device
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    img = image.detach().float()
    a = torch.nan_to_num(alpha.detach().float(), nan=0.0).clamp(0.0, 1.0)
    tau2 = f32(color_tolerance) * f32(color_tolerance)
    pt = f32(motion_penalty) * tau2
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    S = search
    box = lambda v: F.avg_pool2d(v.unsqueeze(1), 2 * patch + 1, 1, patch, divisor_override=1).squeeze(1) if patch else v      # sums; beyond the border: 0
    inside = F.pad(torch.ones(1, H, W, device=dev), (S, S, S, S))                 # 1 where a pixel of the padded neighbour exists
    order = sorted(((dy * dy + dx * dx, dy, dx) for dy in range(-S, S + 1) for dx in range(-S, S + 1)))
    frames = torch.arange(B, device=dev)
    clip = frames // (clip_len if clip_len else B)
    num, den = a.clone(), torch.ones_like(a)
    for k in [-j for j in range(1, radius + 1)] + list(range(1, radius + 1)):
        t = frames[(frames + k >= 0) & (frames + k < B)]
        t = t[clip[t] == clip[t + k]]
        if t.numel() == 0:
            continue
        It = img[t]
        Is = F.pad(img[t + k], (0, 0, S, S, S, S))
        As = F.pad(a[t + k], (S, S, S, S))
        best_c = torch.zeros(t.numel(), H, W, device=dev)
        best_d, best_a = torch.zeros_like(best_c), torch.zeros_like(best_c)
        got = torch.zeros_like(best_c, dtype=torch.bool)
        for dd, dy, dx in order:
            ys, xs = slice(S + dy, S + dy + H), slice(S + dx, S + dx + W)
            ok = inside[:, ys, xs] > 0                                            # q + d exists (q does: it is a pixel of the frame)
            diff = Is[:, ys, xs] - It
            e = torch.where(ok, (diff * diff).sum(-1), zero)
            n = box(ok.float())
            D = box(e) / (3.0 * n)
            C = D + pt * float(dd)
            take = ok & (C == C) & (~got | (C < best_c))
            best_c = torch.where(take, C, best_c)
            best_d = torch.where(take, D, best_d)
            best_a = torch.where(take, As[:, ys, xs], best_a)
            got = got | take
        u = 1.0 - best_d / tau2
        u = torch.where(u > 0, u, zero)
        ck = f32(strength) * (1.0 - f32(float(abs(k))) / float(radius + 1))
        w = torch.where(got, ck * (u * u), zero)
        num[t] += w * best_a
        den[t] += w
    limit = f32(max_change)
    return (a + torch.minimum(torch.maximum(num / den - a, -limit), limit)).clamp(0.0, 1.0)



def defocus_background(image, alpha, fg=None, bg=None, radius_px=16, highlight_gain=0.0, highlight_threshold=0.8):
    """`Engine.defocus_background` in torch fp32, on the tensors' own device (the function defined in include/sdmatte.h): image [B,H,W,3], alpha
    [B,H,W], optional foreground / background colours [B,H,W,3] -> fp32 [B,H,W,3], the subject over its own background out of focus.  Equal to the
    kernels to fp32 rounding; the identities of the header hold here too (a sum of zeros is zero in a convolution as well).  One depthwise convolution
    of the four planes (w C.r, w C.g, w C.b, w) with the 0 / 1 kernel of the closed disc, zero padding: pixels beyond the border do not exist."""
    import torch.nn.functional as F
    from .engine import Engine
    if image.dim() != 4 or image.shape[-1] != 3 or image.numel() == 0:
        raise ValueError(f"defocus_background: image must be a non-empty [B,H,W,3], got {tuple(image.shape)}")
    if tuple(alpha.shape) != tuple(image.shape[:3]):
        raise ValueError(f"defocus_background: alpha must be [B,H,W] = {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
    for name, t in (("fg", fg), ("bg", bg)):
        if t is not None and tuple(t.shape) != tuple(image.shape):
            raise ValueError(f"defocus_background: {name} must be [B,H,W,3] = {tuple(image.shape)}, got {tuple(t.shape)}")
    R, gain, threshold = Engine._check_defocus_params("defocus_background", radius_px, highlight_gain, highlight_threshold)
    dev = image.device
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    img = image.detach().float()
    a = torch.nan_to_num(alpha.detach().float(), nan=0.0).clamp(0.0, 1.0)
    C = bg.detach().float() if bg is not None else img
    Fg = fg.detach().float() if fg is not None else img
    Y = ((C[..., 0] + C[..., 1]) + C[..., 2]) / 3.0
    w = (1.0 - a) * (1.0 + f32(gain) * (Y - f32(threshold)).clamp(min=0.0))
    planes = torch.cat([w.unsqueeze(-1) * C, w.unsqueeze(-1)], -1).permute(0, 3, 1, 2).contiguous()
    d = torch.arange(-R, R + 1, device=dev)
    disc = ((d.view(-1, 1) ** 2 + d.view(1, -1) ** 2) <= R * R).float()
    sums = F.conv2d(planes, disc.expand(4, 1, 2 * R + 1, 2 * R + 1).contiguous(), padding=R, groups=4).permute(0, 2, 3, 1)
    e = f32(2.0 ** -10)      # SDM_DEFOCUS_FLOOR
    blur = (sums[..., :3] + e * C) / (sums[..., 3:].clamp(min=0.0) + e)
    return a.unsqueeze(-1) * Fg + (1.0 - a).unsqueeze(-1) * blur


def clean_plate(image, alpha, bg=None, hole=None, alpha_cut=0.0625, dtype=torch.float32):
    """`Engine.fill_background` in torch, on the tensors' own device (the function defined in include/sdmatte.h): image [B,H,W,3], alpha [B,H,W],
    optional background colours [B,H,W,3] and hole plane [B,H,W] -> [B,H,W,3] in `dtype` (fp32 or fp64), the photo without its subject.  Equal to the
    kernels to fp32 rounding; the identities of the header hold here too.  w_0 is formed in fp32 whatever the dtype, as the contract has it.  The pull
    is four strided slices of a level padded to even sides with zero weights (a missing child adds 0), the push four gathers."""
    import torch.nn.functional as F
    from .engine import Engine
    if image.dim() != 4 or image.shape[-1] != 3 or image.numel() == 0:
        raise ValueError(f"clean_plate: image must be a non-empty [B,H,W,3], got {tuple(image.shape)}")
    if tuple(alpha.shape) != tuple(image.shape[:3]):
        raise ValueError(f"clean_plate: alpha must be [B,H,W] = {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
    if bg is not None and tuple(bg.shape) != tuple(image.shape):
        raise ValueError(f"clean_plate: bg must be [B,H,W,3] = {tuple(image.shape)}, got {tuple(bg.shape)}")
    if hole is not None and tuple(hole.shape) != tuple(alpha.shape):
        raise ValueError(f"clean_plate: hole must be [B,H,W] = {tuple(alpha.shape)}, got {tuple(hole.shape)}")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"clean_plate: dtype must be torch.float32 or torch.float64, got {dtype}")
    cut = Engine._check_f32_range("clean_plate", "alpha_cut", alpha_cut, Engine.PLATE_MIN_CUT, 1)
    dev = image.device
    clean = lambda t: torch.nan_to_num(t.detach().float(), nan=0.0).clamp(0.0, 1.0)
    a = clean(alpha)
    if hole is not None:
        a = torch.maximum(a, clean(hole))
    w = (1.0 - a / torch.tensor(cut, dtype=torch.float32, device=dev)).clamp(0.0, 1.0).to(dtype).unsqueeze(-1)
    C = (bg if bg is not None else image).detach().float().to(dtype)
    levels = [(C, w)]
    while C.shape[1] > 1 or C.shape[2] > 1:
        h, ww = C.shape[1:3]
        pad = (0, 0, 0, ww % 2, 0, h % 2)
        Cp, wp = F.pad(C, pad), F.pad(w, pad)
        kids = [(wp[:, dy::2, dx::2], Cp[:, dy::2, dx::2]) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
        Sw = ((kids[0][0] + kids[1][0]) + kids[2][0]) + kids[3][0]
        Sc = ((kids[0][0] * kids[0][1] + kids[1][0] * kids[1][1]) + kids[2][0] * kids[2][1]) + kids[3][0] * kids[3][1]
        some = Sw > 0
        C = torch.where(some, Sc / torch.where(some, Sw, torch.ones_like(Sw)), torch.zeros_like(Sc))
        w = Sw.clamp(max=1.0)
        levels.append((C, w))
    Fl = levels[-1][0]
    for C, w in reversed(levels[:-1]):
        h, ww = C.shape[1:3]
        hc, wc = Fl.shape[1:3]
        y, x = torch.arange(h, device=dev), torch.arange(ww, device=dev)
        ny, nx = y >> 1, x >> 1
        fy = (ny + (y & 1) * 2 - 1).clamp(0, hc - 1)
        fx = (nx + (x & 1) * 2 - 1).clamp(0, wc - 1)
        Fn, Ff = Fl[:, ny], Fl[:, fy]
        U = 0.75 * (0.75 * Fn[:, :, nx] + 0.25 * Fn[:, :, fx]) + 0.25 * (0.75 * Ff[:, :, nx] + 0.25 * Ff[:, :, fx])
        Fl = w * C + (1.0 - w) * U
    return Fl


def _harmonize_opponent(c):
    return torch.stack([((c[..., 0] + c[..., 1]) + c[..., 2]) / 3.0, c[..., 0] - c[..., 1], (c[..., 0] + c[..., 1]) / 2.0 - c[..., 2]], -1)


def harmonize_map(fg, alpha, bg, luma_strength=0.6, chroma_strength=0.8, contrast_strength=0.5):
    """The colour map of `Engine.harmonize` in torch (the function defined in include/sdmatte.h): fg [B,H,W,3], alpha [B,H,W], bg [1 or B,H,W,3] ->
    fp32 [B,12] on the tensors' device, per image the nine entries of M row-major, then the three of t.  The per-pixel terms are fp32; they are summed
    per image row in fp32, and the row sums and everything after them in fp64 (the kernels sum runs of 4096 pixels instead: equal to fp32 rounding)."""
    from .engine import Engine
    B, H, W = Engine._check_harmonize_shapes("harmonize_map", fg, alpha, bg)
    luma, chroma, contrast, _, _ = Engine._check_harmonize_params("harmonize_map", luma_strength, chroma_strength, contrast_strength, 0.0, 1.0)
    dev = fg.device
    out = torch.zeros(B, 12, dtype=torch.float64, device=dev)
    out[:, 0] = out[:, 4] = out[:, 8] = 1.0
    if luma == 0.0 and chroma == 0.0:
        return out.float()
    F = fg.detach().float()
    a = torch.nan_to_num(alpha.detach().float(), nan=0.0).clamp(0.0, 1.0)
    Bg = bg.detach().float().expand(B, H, W, 3)
    oF, oB = _harmonize_opponent(F), _harmonize_opponent(Bg)
    ao = a.unsqueeze(-1) * oF
    rows = lambda t: t.sum(2).double().sum(1)               # fp32 per row, then fp64
    Wf, n = rows(a), float(H * W)
    ok = Wf >= 1.0                                          # SDM_HZ_MIN_WEIGHT
    Wd = torch.where(ok, Wf, torch.ones_like(Wf)).unsqueeze(-1)
    mf, mb = rows(ao) / Wd, rows(oB) / n
    vf, vb = rows(ao * oF) / Wd - mf * mf, rows(oB * oB) / n - mb * mb
    e = 2.0 ** -20                                          # SDM_HZ_VAR_FLOOR
    s = torch.tensor([luma, chroma, chroma], dtype=torch.float64, device=dev)
    rho = torch.sqrt((vb.clamp(min=0.0) + e) / (vf.clamp(min=0.0) + e)).clamp(0.25, 4.0)      # SDM_HZ_MAX_GAIN; the variances clamped at 0 first
    g = 1.0 + contrast * s * (rho - 1.0)
    h = mf * (1.0 - g) + s * (mb - mf)
    P = torch.tensor([[[1, 1, 1], [1, 1, 1], [1, 1, 1]], [[1.5, -1.5, 0], [-1.5, 1.5, 0], [0, 0, 0]], [[.5, .5, -1], [.5, .5, -1], [-1, -1, 2]]],
                     dtype=torch.float64, device=dev) / 3.0
    K = torch.tensor([[1, 1, 1], [.5, -.5, 0], [1 / 3, 1 / 3, -2 / 3]], dtype=torch.float64, device=dev)
    M = torch.eye(3, dtype=torch.float64, device=dev) + torch.einsum("bc,cij->bij", g - 1.0, P)
    t = torch.einsum("bc,ci->bi", h, K)
    full = torch.cat([M.reshape(B, 9), t], 1)
    return torch.where(ok.unsqueeze(-1), full, out).float()


def harmonize_cutout(fg, alpha, bg, luma_strength=0.6, chroma_strength=0.8, contrast_strength=0.5, wrap_strength=0.5, wrap_sigma=6.0, return_fg=False,
                     return_map=False):
    """`Engine.harmonize` in torch fp32, on the tensors' own device (the function defined in include/sdmatte.h): the straight colours `fg` [B,H,W,3]
    moved towards the colour statistics of the scene `bg` [1 or B,H,W,3], the scene's visible light wrapped over the subject's edge, composed over the
    scene with `alpha` [B,H,W] -> fp32 [B,H,W,3] (and the adjusted colours, and the map [B,12]).  Equal to the kernels to fp32 rounding; the
    identities of the header hold here too.  The wrap is two 1-D convolutions with zero padding, rows first."""
    import math
    import torch.nn.functional as Fn
    from .engine import Engine
    B, H, W = Engine._check_harmonize_shapes("harmonize_cutout", fg, alpha, bg)
    luma, chroma, contrast, wrap, sigma = Engine._check_harmonize_params("harmonize_cutout", luma_strength, chroma_strength, contrast_strength,
                                                                         wrap_strength, wrap_sigma)
    m = harmonize_map(fg, alpha, bg, luma, chroma, contrast)
    F = fg.detach().float()
    a = torch.nan_to_num(alpha.detach().float(), nan=0.0).clamp(0.0, 1.0)
    Bg = bg.detach().float().expand(B, H, W, 3)
    M, t = m[:, :9].view(B, 1, 1, 3, 3), m[:, 9:].view(B, 1, 1, 3)
    Fp = (((t + M[..., 0] * F[..., 0:1]) + M[..., 1] * F[..., 1:2]) + M[..., 2] * F[..., 2:3]).clamp(0.0, 1.0)
    if wrap > 0.0:
        r = int(math.ceil(3.0 * sigma))
        i = torch.arange(-r, r + 1, dtype=torch.float64)
        w = torch.exp(-(i * i) / (2.0 * sigma * sigma))
        w = (w / w.sum()).float().to(F.device)
        v = 1.0 - a
        X = torch.cat([v.unsqueeze(-1) * Bg, v.unsqueeze(-1)], -1).permute(0, 3, 1, 2).contiguous()
        T = Fn.conv2d(X, w.view(1, 1, 1, -1).expand(4, 1, 1, 2 * r + 1).contiguous(), padding=(0, r), groups=4)
        Wm = Fn.conv2d(T, w.view(1, 1, -1, 1).expand(4, 1, 2 * r + 1, 1).contiguous(), padding=(r, 0), groups=4).permute(0, 2, 3, 1)
        Fp = (Fp + wrap * (Wm[..., :3] - Wm[..., 3:] * Fp)).clamp(0.0, 1.0)
    out = a.unsqueeze(-1) * Fp + (1.0 - a).unsqueeze(-1) * Bg
    res = (out, ) + ((Fp, ) if return_fg else ()) + ((m, ) if return_map else ())
    return res[0] if len(res) == 1 else res


def _key_dtype(what, dtype):
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: dtype must be torch.float32 or torch.float64, got {dtype}")
    return dtype


def _key_bins(image, hint):
    """(eligible [B,H,W] bool, iu, iv int64 [B,H,W]) of sdm_screen_colour: fp32 whatever comes after, as the contract has it."""
    r, g, b = image.detach().float().unbind(-1)
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=image.device)
    s = (r + g) + b
    mx = torch.where(g > r, g, r)
    mx = torch.where(b > mx, b, mx)
    mn = torch.where(g < r, g, r)
    mn = torch.where(b < mn, b, mn)
    ok = (s >= f(0.15)) & ((mx - mn) >= f(0.25) * s)
    if hint == 1:
        ok = ok & (g > r) & (g > b)
    if hint == 2:
        ok = ok & (b > r) & (b > g)

    def index(c):
        u = (c / s) * f(64.0)
        return torch.where(u >= 0, torch.where(u < 64, u, f(63.0)), f(0.0)).to(torch.int64)
    return ok, index(r), index(g)


def screen_colour(image, hint="green", share=False, return_info=False, dtype=torch.float32):
    """`Engine.screen_colour` in torch, on the tensor's own device (the function defined in include/sdmatte.h): image [B,H,W,3] -> the screen's colour
    [B,3] in `dtype` (fp32 or fp64), with return_info also int32 [B,4] = {eligible pixels, selected pixels, iu, iv}.  The histogram, the mode and the
    info are exact; the colour is equal to the kernels' to fp32 rounding (fp32: sums per run of 4096 pixels, then fp64, as the contract has it)."""
    import torch.nn.functional as F
    from .engine import Engine
    B, H, W = Engine._check_key_image("screen_colour", image)
    hint = Engine._check_key_hint("screen_colour", hint)
    dtype = _key_dtype("screen_colour", dtype)
    dev = image.device
    ok, iu, iv = _key_bins(image, hint)
    slots = 1 if share else B
    c = image.detach().float().reshape(slots, -1, 3)
    ok, iu, iv = ok.reshape(slots, -1), iu.reshape(slots, -1), iv.reshape(slots, -1)
    P = c.shape[1]
    colour = torch.zeros(slots, 3, dtype=dtype, device=dev)
    info = torch.zeros(slots, 4, dtype=torch.int32, device=dev)
    for s in range(slots):
        idx = (iu[s] * 64 + iv[s])[ok[s]]
        if idx.numel() == 0:
            info[s, 2:] = -1
            continue
        hist = torch.bincount(idx, minlength=4096).view(64, 64)
        pad = F.pad(hist, (1, 1, 1, 1))
        C = sum(pad[dy:dy + 64, dx:dx + 64] for dy in range(3) for dx in range(3)).flatten()
        mode = int((C == C.max()).nonzero()[0])
        mu, mv = mode // 64, mode % 64
        sel = ok[s] & ((iu[s] - mu).abs() <= 1) & ((iv[s] - mv).abs() <= 1)
        n = int(sel.sum())
        vals = torch.where(sel.unsqueeze(-1), c[s], torch.zeros_like(c[s])).to(dtype)
        runs = -(-P // 4096)
        vals = F.pad(vals, (0, 0, 0, runs * 4096 - P)).view(runs, 4096, 3)
        colour[s] = (vals.sum(dim=1).double().sum(dim=0) / n).to(dtype)
        info[s] = torch.tensor([int(ok[s].sum()), n, mu, mv], dtype=torch.int32, device=dev)
    if share:
        colour, info = colour.expand(B, 3).contiguous(), info.expand(B, 4).contiguous()
    return (colour, info) if return_info else colour


def chroma_key(image, screen, clip_fg=0.15, clip_bg=0.85, sure_fg=0.05, sure_bg=0.95, erode_px=10, dilate_px=10, despill=1.0,
               want=("key", "trimap", "despilled"), dtype=torch.float32):
    """`Engine.chroma_key` in torch, on the tensors' own device (the function defined in include/sdmatte.h): image [B,H,W,3] and its screen ([B,3],
    [B,1,1,3] or a colour per pixel [B,H,W,3]) -> the outputs named in `want`, in that order (one name: the tensor itself): key [B,H,W], trimap
    [B,H,W] (through `trimap_from_mask`), despilled [B,H,W,3].  In fp32 equal to the kernels bit for bit; fp64 evaluates the same formulas on the fp32
    inputs and parameters in double."""
    from .engine import Engine
    B, H, W = Engine._check_key_image("chroma_key", image)
    screen, _ = Engine._check_key_screen("chroma_key", screen, B, H, W)
    cf, cb, sf, sb, erode_px, dilate_px, ds = Engine._check_key_params("chroma_key", clip_fg, clip_bg, sure_fg, sure_bg, erode_px, dilate_px, despill)
    want = Engine._check_key_want("chroma_key", want)
    dtype = _key_dtype("chroma_key", dtype)
    dev = image.device
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=dev).to(dtype)
    img = image.detach().float().to(dtype)
    S = screen.detach().float().to(dtype)
    S = (S.view(B, 1, 1, 3) if S.dim() == 2 else S).expand(B, H, W, 3)
    k = torch.where(S[..., 1] > S[..., 0], 1, 0)
    k = torch.where(S[..., 2] > torch.where(k == 1, S[..., 1], S[..., 0]), 2, k)

    def split(v):
        r, g, b = v.unbind(-1)
        top = torch.where(k == 0, r, torch.where(k == 1, g, b))
        other = torch.where(k == 0, torch.where(g > b, g, b), torch.where(k == 1, torch.where(r > b, r, b), torch.where(r > g, r, g)))
        return top, other
    ck, yc = split(img)
    Sk, yS = split(S)
    m, mS = ck - yc, Sk - yS
    valid = (mS >= f(Engine.KEY_MIN_SEP)) & torch.isfinite(m)
    q = (f(cb) * mS - m) / ((f(cb) - f(cf)) * mS)
    one, zero = torch.ones_like(q), torch.zeros_like(q)
    key = torch.where(valid, torch.where(q > 0, torch.where(q < 1, q, one), zero), one)
    cls_f = valid & (m <= f(sf) * mS)
    cls_b = valid & ~cls_f & (m >= f(sb) * mS)
    outs = {"key": key}
    if "trimap" in want:
        t0 = trimap_from_mask(key, 0.5, erode_px, dilate_px).to(dev)
        keep = ((t0 == 1.0) & cls_f) | ((t0 == 0.0) & cls_b) | (t0 == 0.5)
        outs["trimap"] = torch.where(keep, t0, torch.full_like(t0, 0.5)).to(dtype)
    if "despilled" in want:
        d = ck - f(ds) * m
        spill = valid & (m > 0)
        outs["despilled"] = torch.stack([torch.where(spill & (k == c), d, img[..., c]) for c in range(3)], dim=-1)
    res = tuple(outs[w] for w in want)
    return res[0] if len(res) == 1 else res


def key_screen(image, hint="green", share=False, screen_correction=True, screen_cut=0.25, clip_fg=0.15, clip_bg=0.85, sure_fg=0.05, sure_bg=0.95,
               erode_px=10, dilate_px=10, despill=1.0, want=("key", "trimap", "despilled"), dtype=torch.float32):
    """`Engine.key_screen` in torch: `screen_colour`, then `chroma_key`; with screen_correction a first key, `clean_plate(image, key, alpha_cut =
    screen_cut)` as the screen's colour at each pixel, and the key against that plane.  Returns the outputs named in `want`, then the screen ([B,3]
    or the plate [B,H,W,3])."""
    params = (clip_fg, clip_bg, sure_fg, sure_bg, erode_px, dilate_px, despill)
    screen = screen_colour(image, hint, share, dtype=dtype)
    if screen_correction:
        key = chroma_key(image, screen.float(), *params, want=("key", ), dtype=dtype)
        screen = clean_plate(image, key.float(), alpha_cut=screen_cut, dtype=dtype)
    res = chroma_key(image, screen.float(), *params, want=want, dtype=dtype)
    return (res if isinstance(res, tuple) else (res, )) + (screen, )


def matte_metric_weights(grad_sigma=1.4):
    """(r, G, D) of sdm_matte_metrics: the Gaussian and its derivative for offsets -r .. r, computed in double from the fp32 sigma, scaled so that G (x) D
    has unit L2 norm, rounded to fp32 (numpy arrays)."""
    import numpy as np
    s = float(np.float32(grad_sigma))
    r = min(9, max(1, int(np.ceil(s * np.sqrt(-2.0 * np.log(np.sqrt(2.0 * np.pi) * s * 0.01))))))
    i = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * s * s)) / (s * np.sqrt(2.0 * np.pi))
    d = -i * g / (s * s)
    norm = np.sqrt(np.sqrt((g * g).sum() * (d * d).sum()))
    return r, (g / norm).astype(np.float32), (d / norm).astype(np.float32)


def _gradient_magnitude(a, r, G, D):
    """a [B,H,W] -> m(a) of sdm_matte_metrics in a's dtype: replicate padding, the inner sums over the rows first, both sums ascending."""
    B, H, W = a.shape
    pad = torch.nn.functional.pad(a.unsqueeze(1), (r, r, r, r), mode="replicate")[:, 0]
    vg = torch.zeros(B, H, W + 2 * r, dtype=a.dtype, device=a.device)
    vd = torch.zeros_like(vg)
    for k in range(2 * r + 1):
        vg = vg + float(G[k]) * pad[:, k:k + H, :]
        vd = vd + float(D[k]) * pad[:, k:k + H, :]
    ax = torch.zeros(B, H, W, dtype=a.dtype, device=a.device)
    ay = torch.zeros_like(ax)
    for k in range(2 * r + 1):
        ax = ax + float(D[k]) * vg[:, :, k:k + W]
        ay = ay + float(G[k]) * vd[:, :, k:k + W]
    return torch.sqrt(ax * ax + ay * ay)


def connectivity_levels(c):
    """c = min(p, g) [B,H,W] -> int32 [B,H,W]: the level map L of sdm_matte_metrics, exact (compares, counts and `_component_roots` only).  Level k's
    set is c >= (float)k / 10.0f; its largest 4-connected component (the smallest root on a tie) keeps the pixels that reached level k - 1."""
    import numpy as np
    cn = c.detach().cpu().numpy()
    B, H, W = cn.shape
    L = np.zeros((B, H, W), np.int32)
    for k in range(1, 11):
        t = np.float32(k) / np.float32(10.0)
        for b in range(B):
            cls = cn[b] >= t
            if not cls.any():
                continue
            roots = _component_roots(cls, False)
            area = np.bincount(roots[cls], minlength=H * W)
            keep = int(np.argmax(area))                       # the first maximum: the smallest root among the largest components
            L[b][(L[b] == k - 1) & (roots == keep)] = k
    return torch.from_numpy(L).to(c.device)


def matte_metrics(pred, gt, trimap=None, grad_sigma=1.4, conn=True, return_levels=False):
    """`Engine.matte_metrics` in torch, on the tensors' device (the labelling alone goes through numpy on the CPU; the definition is in include/sdmatte.h, sdm_matte_metrics), with the same return value: a dict of
    fp64 tensors [B] `n`, `sad`, `mse`, `grad`, `conn`, `max_abs`, `sad_frame`, `mse_frame` in the literature's units, `raw` [B,8], and `levels` with
    return_levels.  The terms and their sums are formed in the dtype of `pred` (fp32 or fp64), so the function is both the fp32 restatement and the
    fp64 reference; the band test, the thresholds, theta and the filter weights are the fp32 values of the definition in either case, and the level map
    is exact."""
    import numpy as np
    if pred.dim() != 3 or pred.numel() == 0 or gt.shape != pred.shape or (trimap is not None and trimap.shape != pred.shape):
        raise ValueError(f"matte_metrics: pred, gt and trimap must be equal non-empty [B,H,W], got {tuple(pred.shape)}, {tuple(gt.shape)}"
                         + (f", {tuple(trimap.shape)}" if trimap is not None else ""))
    if return_levels and not conn:
        raise ValueError("matte_metrics: return_levels needs conn=True")
    sigma = float(np.float32(grad_sigma))
    if not (np.isfinite(sigma) and 0.25 <= sigma <= 4.0):
        raise ValueError(f"matte_metrics: grad_sigma must be a finite number in [0.25, 4], got {grad_sigma!r}")
    dt = pred.dtype if pred.dtype in (torch.float32, torch.float64) else torch.float32
    B, H, W = (int(v) for v in pred.shape)
    dev = pred.device
    clean = lambda t: torch.clamp(torch.nan_to_num(t.detach().to(dt), nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)
    p, g = clean(pred), clean(gt)
    region = torch.ones(B, H, W, dtype=torch.bool, device=dev) if trimap is None else ((trimap.detach().float() - 0.5).abs() < 0.25)
    e = p - g
    ae, ee = e.abs(), e * e
    r, G, D = matte_metric_weights(sigma)
    dm = _gradient_magnitude(p, r, G, D) - _gradient_magnitude(g, r, G, D)
    zero = torch.zeros((), dtype=dt, device=dev)
    over = lambda t: torch.where(region, t, zero).reshape(B, -1).sum(1)
    raw = torch.zeros(B, 8, dtype=torch.float64, device=dev)
    raw[:, 0] = region.reshape(B, -1).sum(1).double()
    raw[:, 1], raw[:, 2], raw[:, 3] = over(ae).double(), over(ee).double(), over(dm * dm).double()
    raw[:, 5] = torch.where(region, ae, zero).reshape(B, -1).max(1).values.double()
    raw[:, 6], raw[:, 7] = ae.reshape(B, -1).sum(1).double(), ee.reshape(B, -1).sum(1).double()
    levels = None
    if conn:
        levels = connectivity_levels(torch.minimum(p, g))
        l = (levels.float() / 10.0).to(dt)                    # t_L: a true fp32 division
        theta = float(np.float32(0.15))

        def phi(a):
            d = a - l
            return 1.0 - torch.where(d >= theta, d, zero)
        raw[:, 4] = over((phi(p) - phi(g)).abs()).double()
    from .engine import Engine
    res = Engine.metrics_from_raw(raw, H * W)              # the literature's units: one definition for the call and its restatement
    if return_levels:
        res["levels"] = levels
    return res


def metrics_report(res):
    """(text, means) of a `matte_metrics` result: one line per image and a mean line; means = (sad, mse, grad, conn) as floats."""
    rows = [[float(res[k][b]) for k in ("sad", "mse", "grad", "conn")] for b in range(int(res["n"].shape[0]))]
    lines = [f"image {b}: SAD {r[0]:.4f}  MSE {r[1]:.6f}  Grad {r[2]:.4f}  Conn {r[3]:.4f}  (n = {int(res['n'][b])}, max|e| = {float(res['max_abs'][b]):.4f})"
             for b, r in enumerate(rows)]
    means = tuple(sum(r[i] for r in rows) / len(rows) for i in range(4))
    lines.append(f"mean: SAD {means[0]:.4f}  MSE {means[1]:.6f}  Grad {means[2]:.4f}  Conn {means[3]:.4f}")
    return "\n".join(lines), means


def fit_background(bg, H, W):
    """bg [N,h,w,3] -> [N,H,W,3]: scaled (bilinear, antialiased) to cover H x W, then centre-cropped; returned as it is when the size is right."""
    import torch.nn.functional as Fn
    if bg.dim() != 4 or bg.shape[-1] != 3 or bg.numel() == 0:
        raise ValueError(f"[SDMatte] background must be a non-empty [N,h,w,3], got {tuple(bg.shape)}")
    h, w = int(bg.shape[1]), int(bg.shape[2])
    if (h, w) == (H, W):
        return bg.float()
    scale = max(H / h, W / w)
    nh, nw = max(H, int(round(h * scale))), max(W, int(round(w * scale)))
    t = bg.float()
    if (nh, nw) != (h, w):
        t = Fn.interpolate(t.permute(0, 3, 1, 2), size=(nh, nw), mode="bilinear", align_corners=False, antialias=True).permute(0, 2, 3, 1)
    y0, x0 = (nh - H) // 2, (nw - W) // 2
    return t[:, y0:y0 + H, x0:x0 + W].clamp(0.0, 1.0).contiguous()


class SDMatteApply:

    @classmethod
    def INPUT_TYPES(s):
        return {
            "required": {
                "ckpt_name": (list(MODEL_URLS.keys()), ),
                "image": ("IMAGE", {"tooltip": "image to matte"}),
                "trimap": ("MASK", {"tooltip": "trimap: white = foreground, black = background, gray = unknown"}),
                "inference_size": ([512, 640, 768, 896, 1024], {"default": 1024, "tooltip": "inference resolution: higher = better and slower (1024 best quality, 768 balanced)"}),
                "is_transparent": ("BOOLEAN", {"default": False, "tooltip": "enable when the source image has a transparent background / depicts a transparent object"}),
                "output_mode": (["alpha_only", "matted_rgba", "matted_rgb"], {"default": "alpha_only", "tooltip": "alpha_only = mask only; matted_rgba = cut-out on a transparent background; matted_rgb = cut-out on black"}),
                "mask_refine": ("BOOLEAN", {"default": True, "tooltip": "refine the mask with the trimap: filters unwanted regions, less background interference"}),
                "trimap_constraint": ("FLOAT", {"default": 0.8, "min": 0.1, "max": 1.0, "step": 0.1, "tooltip": "strength of the trimap constraint (0.1-1.0): higher = stricter; 0.8 balanced, 0.9 strict, 0.6 permissive"}),
            },
            "optional": {
                "force_cpu": ("BOOLEAN", {"default": False}),
            },
        }

    RETURN_TYPES = ("MASK", "IMAGE")
    RETURN_NAMES = ("alpha_mask", "matted_image")
    FUNCTION = "apply_matte"
    CATEGORY = "Matting/SDMatte"

    def apply_matte(self, ckpt_name, image, trimap, inference_size, is_transparent, output_mode, mask_refine, trimap_constraint,
                    force_cpu=False):
        if force_cpu:
            raise RuntimeError("[SDMatte] force_cpu=True is not available: this node runs hand-written gfx950 kernels only "
                               "(no CPU path).  Use the reference plugin for CPU inference.")
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        # the trimap is resized to the inference size on its own, as in the reference (sdmatte_nodes.py:212-214,349); its size only has
        # to equal the image's where the reference indexes the alpha with it (mask_refine, matted_rgb): the engine raises there
        if trimap.dim() != 3 or trimap.shape[0] != image.shape[0]:
            raise ValueError(f"[SDMatte] trimap must be [B,h,w] with the image's batch size, got {tuple(trimap.shape)}")
        model = get_model(ckpt_name, _torch_device())
        fan = _fan_out(model, image.shape[0])
        # one C-ABI call per device: resize / normalise / model / resize back / clamp AND mask_refine + output composition, all on
        # the GPU at the original resolution (bit-identical to the reference's CPU tail, tests/test_emu_e2e.py); with several GPUs
        # the batch is split over them (one engine + host thread per device)
        runner = fan if fan is not None else model.engine
        out, matted = runner.apply_matte_node(image, trimap, int(inference_size), bool(is_transparent), output_mode, bool(mask_refine),
                                              float(trimap_constraint))
        out, matted = out.detach().cpu(), matted.detach().cpu()
        _trim_engine_memory(model)
        return (out, matted)


_TRIMAP_INPUTS = {
    "threshold": ("FLOAT", {"default": 0.5, "min": 0.0, "max": 1.0, "step": 0.01, "tooltip": "mask values above this are foreground"}),
    "erode_px": ("INT", {"default": 10, "min": 0, "max": 255, "step": 1, "tooltip": "foreground closer than this to the mask's edge becomes unknown (pixels)"}),
    "dilate_px": ("INT", {"default": 10, "min": 0, "max": 255, "step": 1, "tooltip": "background closer than this to the mask becomes unknown (pixels)"}),
}


class SDMatteTrimapFromMask:
    """Mask (SAM, RMBG, a hand-drawn selection) -> trimap, on the GPU; needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": dict({"mask": ("MASK", {"tooltip": "mask to turn into a trimap"})}, **_TRIMAP_INPUTS)}

    RETURN_TYPES = ("MASK", )
    RETURN_NAMES = ("trimap", )
    FUNCTION = "make_trimap"
    CATEGORY = "Matting/SDMatte"

    def make_trimap(self, mask, threshold=0.5, erode_px=10, dilate_px=10):
        if mask.dim() == 2:
            mask = mask.unsqueeze(0)
        if mask.dim() != 3:
            raise ValueError(f"[SDMatte] mask must be [B,H,W], got {tuple(mask.shape)}")
        eng = _trimap_engine(_torch_device())
        return (eng.make_trimap(mask.detach().cpu(), float(threshold), int(erode_px), int(dilate_px)), )


_CLEAN_INPUTS = {
    "threshold": ("FLOAT", {"default": 0.5, "min": 0.0, "max": 0.99, "step": 0.01, "tooltip": "mask values above this are foreground"}),
    "min_area": ("INT", {"default": 64, "min": 0, "max": 1 << 28, "step": 1, "tooltip": "foreground islands of fewer pixels are removed (0 or 1: none)"}),
    "keep_largest": ("BOOLEAN", {"default": False, "tooltip": "keep only the largest foreground component"}),
    "max_hole_area": ("INT", {"default": 64, "min": 0, "max": 1 << 28, "step": 1, "tooltip": "holes of at most this many pixels are filled (0: none)"}),
    "binarize": ("BOOLEAN", {"default": False, "tooltip": "return 1.0 / 0.0 instead of the mask's own values where nothing changed"}),
}


class SDMatteCleanMask:
    """Mask -> the mask without stray islands and pin-holes (optionally: only its largest component), on the GPU, for the trimap node after it;
    needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": dict({"mask": ("MASK", {"tooltip": "mask to clean (SAM, RMBG, a selection)"})}, **_CLEAN_INPUTS)}

    RETURN_TYPES = ("MASK", )
    RETURN_NAMES = ("mask", )
    FUNCTION = "clean"
    CATEGORY = "Matting/SDMatte"

    def clean(self, mask, threshold=0.5, min_area=64, keep_largest=False, max_hole_area=64, binarize=False):
        if mask.dim() == 2:
            mask = mask.unsqueeze(0)
        if mask.dim() != 3 or mask.numel() == 0:
            raise ValueError(f"[SDMatte] mask must be a non-empty [B,H,W], got {tuple(mask.shape)}")
        if not 0.0 <= float(threshold) < 1.0:
            raise ValueError(f"[SDMatte] threshold must be in [0, 1), got {threshold!r}")
        for name, v in (("min_area", min_area), ("max_hole_area", max_hole_area)):
            if int(v) != v or not 0 <= int(v) <= (1 << 28):
                raise ValueError(f"[SDMatte] {name} must be an integer in 0 .. {1 << 28}, got {v!r}")
        eng = _trimap_engine(_torch_device())
        return (eng.clean_mask(mask.detach().cpu(), float(threshold), int(min_area), bool(keep_largest), int(max_hole_area), bool(binarize)), )


class SDMatteApplyMask:
    """`Apply SDMatte` fed with a mask: the trimap is made from it on the GPU inside the same engine call, and returned as well."""

    @classmethod
    def INPUT_TYPES(s):
        base = SDMatteApply.INPUT_TYPES()
        required = {}
        for key, spec in base["required"].items():
            if key == "trimap":
                required["mask"] = ("MASK", {"tooltip": "mask of the object: the trimap is made from it (threshold, erode_px, dilate_px)"})
                required.update(_TRIMAP_INPUTS)
            else:
                required[key] = spec
        return {"required": required, "optional": base["optional"]}

    RETURN_TYPES = ("MASK", "IMAGE", "MASK")
    RETURN_NAMES = ("alpha_mask", "matted_image", "trimap")
    FUNCTION = "apply_matte"
    CATEGORY = "Matting/SDMatte"

    def apply_matte(self, ckpt_name, image, mask, threshold, erode_px, dilate_px, inference_size, is_transparent, output_mode, mask_refine,
                    trimap_constraint, force_cpu=False):
        if force_cpu:
            raise RuntimeError("[SDMatte] force_cpu=True is not available: this node runs hand-written gfx950 kernels only "
                               "(no CPU path).  Use the reference plugin for CPU inference.")
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if mask.dim() != 3 or mask.shape[0] != image.shape[0]:
            raise ValueError(f"[SDMatte] mask must be [B,h,w] with the image's batch size, got {tuple(mask.shape)}")
        model = get_model(ckpt_name, _torch_device())
        fan = _fan_out(model, image.shape[0])
        runner = fan if fan is not None else model.engine
        out, matted, trimap = runner.apply_matte_mask(image, mask, int(inference_size), bool(is_transparent), output_mode, bool(mask_refine),
                                                      float(trimap_constraint), float(threshold), int(erode_px), int(dilate_px))
        out, matted, trimap = out.detach().cpu(), matted.detach().cpu(), trimap.detach().cpu()
        _trim_engine_memory(model)
        return (out, matted, trimap)


_ROI_INPUTS = {
    "roi_threshold": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 0.99, "step": 0.01, "tooltip": "trimap values above this belong to the subject (0 = everything but definite background)"}),
    "margin_px": ("INT", {"default": 16, "min": 0, "max": 4096, "step": 1, "tooltip": "context around the subject's box, in pixels per side"}),
    "margin_pct": ("INT", {"default": 10, "min": 0, "max": 100, "step": 1, "tooltip": "... plus this many percent of the box's extent per side"}),
    "square": ("BOOLEAN", {"default": True, "tooltip": "grow the box to a square where the frame allows (the model's input is square)"}),
}


class SDMatteApplyROI:
    """`Apply SDMatte (Mask)` on the subject instead of the frame: the model sees the box of the trimap at `inference_size`, the alpha outside the box
    is 0 (exact: the trimap is definite background there).  Returns the box as well: one (x, y, width, height) per image."""

    @classmethod
    def INPUT_TYPES(s):
        base = SDMatteApplyMask.INPUT_TYPES()
        required = {}
        for key, spec in base["required"].items():
            required[key] = spec
            if key == "dilate_px":
                required.update(_ROI_INPUTS)
        return {"required": required, "optional": base["optional"]}

    RETURN_TYPES = ("MASK", "IMAGE", "MASK", "BBOX")
    RETURN_NAMES = ("alpha_mask", "matted_image", "trimap", "roi")
    FUNCTION = "apply_matte"
    CATEGORY = "Matting/SDMatte"

    def apply_matte(self, ckpt_name, image, mask, threshold, erode_px, dilate_px, roi_threshold, margin_px, margin_pct, square, inference_size,
                    is_transparent, output_mode, mask_refine, trimap_constraint, force_cpu=False):
        from .engine import Engine
        if force_cpu:
            raise RuntimeError("[SDMatte] force_cpu=True is not available: this node runs hand-written gfx950 kernels only "
                               "(no CPU path).  Use the reference plugin for CPU inference.")
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if mask.dim() != 3 or tuple(mask.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] mask must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(mask.shape)}")
        Engine._check_roi_params("[SDMatte] apply_matte", roi_threshold, margin_px, margin_pct)
        model = get_model(ckpt_name, _torch_device())
        fan = _fan_out(model, image.shape[0])
        runner = fan if fan is not None else model.engine
        out, matted, trimap, roi = runner.apply_matte_roi(image, mask, int(inference_size), bool(is_transparent), output_mode, bool(mask_refine),
                                                          float(trimap_constraint), True, float(threshold), int(erode_px), int(dilate_px),
                                                          float(roi_threshold), int(margin_px), int(margin_pct), bool(square))
        out, matted, trimap = out.detach().cpu(), matted.detach().cpu(), trimap.detach().cpu()
        boxes = [(int(x0), int(y0), int(w), int(h)) for y0, x0, h, w in roi.detach().cpu().tolist()]
        _trim_engine_memory(model)
        return (out, matted, trimap, boxes)


_SUBJECTS_INPUTS = {
    "max_subjects": ("INT", {"default": 4, "min": 1, "max": 8, "step": 1, "tooltip": "boxes per image: the largest subjects get one each, the last one takes whatever is left"}),
    "min_area": ("INT", {"default": 64, "min": 0, "max": 1 << 28, "step": 1, "tooltip": "a component of the trimap below this many pixels gets no box of its own"}),
}


def split_boxes(boxes, B, limit):
    """Consecutive image ranges (lo, hi, entries) such that no range has more than `limit` entries: entries int32 [n,5] of the images lo .. hi-1 with b
    rebased to the range.  `boxes` is a compacted list whose entries are grouped by image in ascending order."""
    per = [boxes[boxes[:, 0] == b] for b in range(B)]
    out, lo, n = [], 0, 0
    for b in range(B):
        if len(per[b]) > limit:
            raise ValueError(f"split_boxes: image {b} has {len(per[b])} boxes, more than {limit}")
        if n + len(per[b]) > limit:
            out.append((lo, b))
            lo, n = b, 0
        n += len(per[b])
    out.append((lo, B))
    res = []
    for lo, hi in out:
        part = torch.cat(per[lo:hi]).clone()
        part[:, 0] -= lo
        res.append((lo, hi, part.contiguous()))
    return res


class SDMatteApplySubjects:
    """`Apply SDMatte (Subject Box)` with a box per subject: every large component of the trimap is matted in a model pass of its own at `inference_size`,
    and the passes are merged by their maximum.  Returns the boxes as well: a list of (x, y, width, height) per image."""

    @classmethod
    def INPUT_TYPES(s):
        base = SDMatteApplyROI.INPUT_TYPES()
        required = {}
        for key, spec in base["required"].items():
            required[key] = spec
            if key == "square":
                required.update(_SUBJECTS_INPUTS)
        return {"required": required, "optional": base["optional"]}

    RETURN_TYPES = ("MASK", "IMAGE", "MASK", "BBOX")
    RETURN_NAMES = ("alpha_mask", "matted_image", "trimap", "boxes")
    FUNCTION = "apply_matte"
    CATEGORY = "Matting/SDMatte"

    def apply_matte(self, ckpt_name, image, mask, threshold, erode_px, dilate_px, roi_threshold, margin_px, margin_pct, square, max_subjects, min_area,
                    inference_size, is_transparent, output_mode, mask_refine, trimap_constraint, force_cpu=False):
        from .engine import Engine
        if force_cpu:
            raise RuntimeError("[SDMatte] force_cpu=True is not available: this node runs hand-written gfx950 kernels only "
                               "(no CPU path).  Use the reference plugin for CPU inference.")
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if mask.dim() != 3 or tuple(mask.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] mask must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(mask.shape)}")
        Engine._check_roi_params("[SDMatte] apply_matte", roi_threshold, margin_px, margin_pct)
        Engine._check_boxes_params("[SDMatte] apply_matte", min_area, max_subjects)
        return self._run(get_model(ckpt_name, _torch_device()), image, mask, float(threshold), int(erode_px), int(dilate_px), float(roi_threshold),
                         int(margin_px), int(margin_pct), bool(square), int(max_subjects), int(min_area), int(inference_size), bool(is_transparent),
                         output_mode, bool(mask_refine), float(trimap_constraint))

    @staticmethod
    def _run(model, image, mask, threshold, erode_px, dilate_px, roi_threshold, margin_px, margin_pct, square, max_subjects, min_area, inference_size,
             is_transparent, output_mode, mask_refine, trimap_constraint):
        """Trimap, boxes, a readback of the few hundred bytes of the list, then one apply_matte_boxes call per range of images with at most
        SDM_BOXES_MAX_TOTAL entries."""
        from .engine import Engine
        eng = model.engine
        B = int(image.shape[0])
        trimap = eng.make_trimap(mask, threshold, erode_px, dilate_px)
        boxes = compact_boxes(eng.subject_boxes(trimap, roi_threshold, min_area, max_subjects, margin_px, margin_pct, square))
        alphas, matteds = [], []
        for lo, hi, part in split_boxes(boxes, B, Engine.BOXES_MAX_TOTAL):
            fan = _fan_out(model, hi - lo)
            runner = fan if fan is not None else eng
            a, m = runner.apply_matte_boxes(image[lo:hi], trimap[lo:hi], part, inference_size, is_transparent, output_mode, mask_refine, trimap_constraint)
            alphas.append(a.detach().cpu())
            matteds.append(m.detach().cpu())
        out = [[(int(x0), int(y0), int(w), int(h)) for bb, y0, x0, h, w in boxes.tolist() if bb == b] for b in range(B)]
        _trim_engine_memory(model)
        return (torch.cat(alphas), torch.cat(matteds), trimap.detach().cpu(), out)


_TILED_INPUTS = {
    "tile_size": ("INT", {"default": 0, "min": 0, "max": 8192, "step": 64, "tooltip": "side of a tile in frame pixels; 0 = the smallest multiple of 64 >= inference_size whose grid has at most 16 tiles"}),
    "overlap": ("INT", {"default": 128, "min": 0, "max": 4096, "step": 1, "tooltip": "neighbouring tiles share at least this many pixels (at most half a tile)"}),
    "feather": ("INT", {"default": -1, "min": -1, "max": 1024, "step": 1, "tooltip": "width of the ramp that blends overlapping tiles; -1 = the overlap"}),
    "band_lo": ("FLOAT", {"default": 0.25, "min": 0.0, "max": 0.99, "step": 0.01, "tooltip": "a tile needs the model if it holds a trimap value above this ..."}),
    "band_hi": ("FLOAT", {"default": 0.75, "min": 0.01, "max": 1.0, "step": 0.01, "tooltip": "... and below this"}),
}


class SDMatteApplyTiled:
    """`Apply SDMatte (Mask)` at the photo's own resolution: the frame is cut into overlapping tiles, every tile that holds a pixel of the trimap's unknown
    band is matted in a model pass of its own at `inference_size`, and the passes are blended with weights that ramp down towards a tile's edges.
    The definite parts of the trimap cost no pass.  Returns the tiles as well: a list of (x, y, width, height) per image."""

    @classmethod
    def INPUT_TYPES(s):
        base = SDMatteApplyMask.INPUT_TYPES()
        required = {}
        for key, spec in base["required"].items():
            required[key] = spec
            if key == "dilate_px":
                required.update(_TILED_INPUTS)
        optional = dict(base["optional"])
        optional["base_alpha"] = ("MASK", {"tooltip": "alpha for the pixels outside every tile (default: the trimap's definite values)"})
        return {"required": required, "optional": optional}

    RETURN_TYPES = ("MASK", "IMAGE", "MASK", "BBOX")
    RETURN_NAMES = ("alpha_mask", "matted_image", "trimap", "tiles")
    FUNCTION = "apply_matte"
    CATEGORY = "Matting/SDMatte"

    def apply_matte(self, ckpt_name, image, mask, threshold, erode_px, dilate_px, tile_size, overlap, feather, band_lo, band_hi, inference_size,
                    is_transparent, output_mode, mask_refine, trimap_constraint, force_cpu=False, base_alpha=None):
        from .engine import Engine
        if force_cpu:
            raise RuntimeError("[SDMatte] force_cpu=True is not available: this node runs hand-written gfx950 kernels only "
                               "(no CPU path).  Use the reference plugin for CPU inference.")
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if mask.dim() != 3 or tuple(mask.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] mask must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(mask.shape)}")
        if base_alpha is not None and tuple(base_alpha.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] base_alpha must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(base_alpha.shape)}")
        H, W = int(image.shape[1]), int(image.shape[2])
        overlap = int(overlap)
        tile = int(tile_size) if int(tile_size) > 0 else auto_tile(H, W, int(inference_size), overlap, Engine.TILES_MAX)
        feather = overlap if int(feather) < 0 else int(feather)
        Engine._check_tiles_params("[SDMatte] apply_matte", band_lo, band_hi, tile, overlap, Engine.TILES_MAX)
        Engine._check_tiles_grid("[SDMatte] apply_matte", H, W, tile, overlap)
        if not 0 <= feather <= Engine.TILES_MAX_FEATHER:
            raise ValueError(f"[SDMatte] feather must be in 0 .. {Engine.TILES_MAX_FEATHER}, got {feather}")
        return self._run(get_model(ckpt_name, _torch_device()), image, mask, float(threshold), int(erode_px), int(dilate_px), tile, overlap, feather,
                         float(band_lo), float(band_hi), int(inference_size), bool(is_transparent), output_mode, bool(mask_refine), float(trimap_constraint),
                         base_alpha)

    @staticmethod
    def _run(model, image, mask, threshold, erode_px, dilate_px, tile, overlap, feather, band_lo, band_hi, inference_size, is_transparent, output_mode,
             mask_refine, trimap_constraint, base_alpha=None):
        """Trimap, tiles, a readback of the few hundred bytes of the list, then one apply_matte_tiles call per range of images with at most SDM_TILES_MAX
        entries; a range without an entry (no unknown pixel) is called with N = 0."""
        from .engine import Engine
        eng = model.engine
        B = int(image.shape[0])
        trimap = eng.make_trimap(mask, threshold, erode_px, dilate_px)
        tiles, count = eng.band_tiles(trimap, band_lo, band_hi, tile, overlap, Engine.TILES_MAX, return_count=True)
        if int(count.max()) > Engine.TILES_MAX:
            raise ValueError(f"[SDMatte] an image needs {int(count.max())} tiles of {tile} pixels, more than {Engine.TILES_MAX}: use a larger tile_size (0 chooses one)")
        tiles = compact_boxes(tiles)
        alphas, matteds = [], []
        for lo, hi, part in split_boxes(tiles, B, Engine.TILES_MAX):
            a, m = eng.apply_matte_tiles(image[lo:hi], trimap[lo:hi], part.to(trimap.device), inference_size, is_transparent, output_mode, mask_refine,
                                         trimap_constraint, feather, None if base_alpha is None else base_alpha[lo:hi].to(trimap.device))
            alphas.append(a.detach().cpu())
            matteds.append(m.detach().cpu())
        out = [[(int(x0), int(y0), int(w), int(h)) for bb, y0, x0, h, w in tiles.tolist() if bb == b] for b in range(B)]
        _trim_engine_memory(model)
        return (torch.cat(alphas), torch.cat(matteds), trimap.detach().cpu(), out)


_FOREGROUND_INPUTS = {
    "regularization": ("FLOAT", {"default": 1e-5, "min": 1e-9, "max": 1.0, "step": 1e-6, "tooltip": "smoothness weight between all neighbours (must be above 0)"}),
    "gradient_weight": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 100.0, "step": 0.01, "tooltip": "extra smoothness weight across alpha edges"}),
    "n_small_iters": ("INT", {"default": 10, "min": 1, "max": 64, "step": 1, "tooltip": "iterations on every level up to 32 pixels"}),
    "n_big_iters": ("INT", {"default": 2, "min": 1, "max": 4, "step": 1, "tooltip": "iterations on every larger level"}),
}


class SDMatteForeground:
    """Image + alpha -> foreground and background colours on the GPU: a cut-out without the old background baked into its soft pixels.  Needs no
    checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE", {"tooltip": "the image the alpha was made for"}),
                             "alpha": ("MASK", {"tooltip": "alpha matte of the image (alpha_mask of Apply SDMatte)"})},
                "optional": dict(_FOREGROUND_INPUTS)}

    RETURN_TYPES = ("IMAGE", "IMAGE", "IMAGE")
    RETURN_NAMES = ("foreground", "background", "foreground_rgba")
    FUNCTION = "estimate"
    CATEGORY = "Matting/SDMatte"

    def estimate(self, image, alpha, regularization=1e-5, gradient_weight=1.0, n_small_iters=10, n_big_iters=2):
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if alpha.dim() == 2:
            alpha = alpha.unsqueeze(0)
        if tuple(alpha.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] alpha must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
        eng = _trimap_engine(_torch_device())
        rgba, bg = eng.estimate_foreground(image.detach().cpu(), alpha.detach().cpu(), float(regularization), float(gradient_weight), int(n_small_iters),
                                           int(n_big_iters), rgba=True)
        return (rgba[..., :3].contiguous(), bg, rgba)


class SDMatteRefineAlpha:
    """Image + alpha -> the alpha refined at the image's own resolution on the GPU (the subsampled colour guided filter): what `Apply SDMatte` returns for
    a photo larger than `inference_size` is a bilinear enlargement, whose edges are ramps of max(H, W) / inference_size pixels.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE", {"tooltip": "the image the alpha was made for, at its own resolution"}),
                             "alpha": ("MASK", {"tooltip": "alpha matte of the image (alpha_mask of Apply SDMatte)"}),
                             "inference_size": SDMatteApply.INPUT_TYPES()["required"]["inference_size"]},
                "optional": {
                    "subsample": ("INT", {"default": 0, "min": 0, "max": 16, "step": 1, "tooltip": "factor between the image and the resolution the alpha was made at; 0 = ceil(max(H, W) / inference_size)"}),
                    "radius": ("INT", {"default": 2, "min": 1, "max": 32, "step": 1, "tooltip": "window radius of the fit, in pixels of the subsampled image"}),
                    "eps": ("FLOAT", {"default": 1e-4, "min": 1e-6, "max": 1.0, "step": 1e-6, "tooltip": "regularisation of the fit: larger = smoother, follows the image's edges less"}),
                }}

    RETURN_TYPES = ("MASK", )
    RETURN_NAMES = ("alpha_mask", )
    FUNCTION = "refine"
    CATEGORY = "Matting/SDMatte"

    def refine(self, image, alpha, inference_size=1024, subsample=0, radius=2, eps=1e-4):
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if alpha.dim() == 2:
            alpha = alpha.unsqueeze(0)
        if tuple(alpha.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] alpha must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
        if int(subsample) == 0:
            subsample = auto_subsample(image.shape[1], image.shape[2], int(inference_size))
        eng = _trimap_engine(_torch_device())
        return (eng.refine_alpha_guided(image.detach().cpu(), alpha.detach().cpu(), int(subsample), int(radius), float(eps)), )


_CANVAS_INPUTS = {
    "fill_pct": ("INT", {"default": 80, "min": 1, "max": 100, "step": 1, "tooltip": "share of the canvas (per side) the subject's box is scaled to fill"}),
    "valign": (["center", "top", "bottom"], {"default": "center", "tooltip": "bottom: the subject stands on the lower edge of the fill area"}),
    "background": (["color", "transparent"], {"default": "color", "tooltip": "ignored when a background image is connected"}),
    "bg_red": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01}),
    "bg_green": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01}),
    "bg_blue": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01}),
    "shadow_opacity": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 1.0, "step": 0.01, "tooltip": "0 = no shadow"}),
    "shadow_sigma": ("FLOAT", {"default": 8.0, "min": 0.1, "max": 32.0, "step": 0.1, "tooltip": "softness of the shadow, in canvas pixels"}),
    "shadow_dy": ("INT", {"default": 0, "min": -4096, "max": 4096, "step": 1, "tooltip": "shadow offset downwards, in canvas pixels"}),
    "shadow_dx": ("INT", {"default": 0, "min": -4096, "max": 4096, "step": 1, "tooltip": "shadow offset to the right, in canvas pixels"}),
}


class SDMatteCanvas:
    """Foreground + alpha -> the subject on a canvas of a given size on the GPU: scaled to fill a share of it, centred or on a baseline, over a colour, an
    image or transparency (RGBA), with an optional soft shadow.  Colours are resampled premultiplied, so no fringe.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"foreground": ("IMAGE", {"tooltip": "foreground colours of the cut-out (foreground of SDMatte Foreground Colours, or the image)"}),
                             "alpha": ("MASK", {"tooltip": "alpha matte of the foreground"}),
                             "canvas_width": ("INT", {"default": 1024, "min": 1, "max": 32768, "step": 1}),
                             "canvas_height": ("INT", {"default": 1024, "min": 1, "max": 32768, "step": 1})},
                "optional": dict(_CANVAS_INPUTS, background_image=("IMAGE", {"tooltip": "opaque background at canvas size (one image, or one per foreground)"}),
                                 force_cpu=("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU call"}))}

    RETURN_TYPES = ("IMAGE", )
    RETURN_NAMES = ("image", )
    FUNCTION = "compose"
    CATEGORY = "Matting/SDMatte"

    def compose(self, foreground, alpha, canvas_width, canvas_height, fill_pct=80, valign="center", background="color", bg_red=1.0, bg_green=1.0,
                bg_blue=1.0, shadow_opacity=0.0, shadow_sigma=8.0, shadow_dy=0, shadow_dx=0, background_image=None, force_cpu=False):
        from .engine import Engine
        if foreground.dim() != 4 or foreground.shape[-1] != 3:
            raise ValueError(f"[SDMatte] foreground must be [B,H,W,3], got {tuple(foreground.shape)}")
        if alpha.dim() == 2:
            alpha = alpha.unsqueeze(0)
        if tuple(alpha.shape) != tuple(foreground.shape[:3]):
            raise ValueError(f"[SDMatte] alpha must be [B,H,W] of the foreground {tuple(foreground.shape[:3])}, got {tuple(alpha.shape)}")
        if background not in ("color", "transparent"):
            raise ValueError(f"[SDMatte] unknown background {background!r}")
        B = int(foreground.shape[0])
        Engine._check_canvas_params("[SDMatte] canvas", B, canvas_height, canvas_width, fill_pct, valign, shadow_opacity, shadow_sigma, shadow_dy, shadow_dx)
        if background_image is not None and (background_image.dim() != 4 or tuple(background_image.shape[1:]) != (int(canvas_height), int(canvas_width), 3) or
                                             int(background_image.shape[0]) not in (1, B)):
            raise ValueError(f"[SDMatte] background_image must be [1 or {B},{int(canvas_height)},{int(canvas_width)},3] (it is not resized), "
                             f"got {tuple(background_image.shape)}")
        color = (float(bg_red), float(bg_green), float(bg_blue)) if background == "color" and background_image is None else None
        args = (foreground.detach().cpu(), alpha.detach().cpu(), int(canvas_height), int(canvas_width), int(fill_pct), valign, color,
                background_image.detach().cpu() if background_image is not None else None, float(shadow_opacity), float(shadow_sigma), int(shadow_dy),
                int(shadow_dx))
        if force_cpu:      # an explicit request, never a silent substitute: the same function in torch
            return (compose_canvas(*args), )
        return (_trimap_engine(_torch_device()).compose_canvas(*args), )


class SDMatteOffsetMask:
    """MASK -> MASK: grow, shrink and feather a mask by any number of pixels on the GPU (the exact Euclidean distance transform; no radius cap, one
    pass whatever the radius).  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"mask": ("MASK", {"tooltip": "mask to grow (offset above 0) or shrink (below 0)"}),
                             "offset_px": ("FLOAT", {"default": 0.0, "min": -1024.0, "max": 1024.0, "step": 0.5, "tooltip": "how far the edge moves outwards, in pixels"}),
                             "feather_px": ("FLOAT", {"default": 1.0, "min": 1.0, "max": 1024.0, "step": 0.5, "tooltip": "width of the ramp across the new edge (1 = hard)"})},
                "optional": {"threshold": ("FLOAT", {"default": 0.5, "min": 0.0, "max": 0.99, "step": 0.01, "tooltip": "the mask's foreground is mask > threshold"}),
                             "force_cpu": ("BOOLEAN", {"default": False, "tooltip": "evaluate the numpy / torch restatement on the CPU instead of the GPU call"})}}

    RETURN_TYPES = ("MASK", )
    RETURN_NAMES = ("mask", )
    FUNCTION = "offset"
    CATEGORY = "Matting/SDMatte"

    def offset(self, mask, offset_px, feather_px, threshold=0.5, force_cpu=False):
        if mask.dim() == 2:
            mask = mask.unsqueeze(0)
        args = (mask.detach().cpu(), float(offset_px), float(feather_px), float(threshold))
        if force_cpu:      # an explicit request, never a silent substitute
            return (offset_mask(*args), )
        return (_trimap_engine(_torch_device()).offset_mask(*args), )


class SDMatteOutline:
    """Foreground + alpha -> the cut-out with an outline (the "sticker" stroke) along its silhouette on the GPU, as straight colours and alpha: what
    SDMatte Canvas takes.  The stroke stays inside the frame: place the cut-out on a canvas first to give it room.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"foreground": ("IMAGE", {"tooltip": "foreground colours of the cut-out"}),
                             "alpha": ("MASK", {"tooltip": "alpha matte of the foreground"}),
                             "width_px": ("FLOAT", {"default": 8.0, "min": 0.5, "max": 1024.0, "step": 0.5}),
                             "position": (list(OUTLINE_POSITION), {"default": "outside", "tooltip": "outside: under the subject; center / inside: over it"})},
                "optional": {"red": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01}),
                             "green": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01}),
                             "blue": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01}),
                             "opacity": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01}),
                             "softness_px": ("FLOAT", {"default": 1.0, "min": 1.0, "max": 1024.0, "step": 0.5, "tooltip": "width of the stroke's soft edges (1 = hard)"}),
                             "edge_threshold": ("FLOAT", {"default": 0.5, "min": 0.0, "max": 0.99, "step": 0.01, "tooltip": "the silhouette is that of alpha > edge_threshold"}),
                             "force_cpu": ("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU call"})}}

    RETURN_TYPES = ("IMAGE", "MASK")
    RETURN_NAMES = ("foreground", "alpha")
    FUNCTION = "outline"
    CATEGORY = "Matting/SDMatte"

    def outline(self, foreground, alpha, width_px, position, red=1.0, green=1.0, blue=1.0, opacity=1.0, softness_px=1.0, edge_threshold=0.5, force_cpu=False):
        if foreground.dim() != 4 or foreground.shape[-1] != 3:
            raise ValueError(f"[SDMatte] foreground must be [B,H,W,3], got {tuple(foreground.shape)}")
        if alpha.dim() == 2:
            alpha = alpha.unsqueeze(0)
        if tuple(alpha.shape) != tuple(foreground.shape[:3]):
            raise ValueError(f"[SDMatte] alpha must be [B,H,W] of the foreground {tuple(foreground.shape[:3])}, got {tuple(alpha.shape)}")
        args = (foreground.detach().cpu(), alpha.detach().cpu(), float(width_px), (float(red), float(green), float(blue)), position, float(softness_px),
                float(opacity), float(edge_threshold))
        if force_cpu:      # an explicit request, never a silent substitute
            return outline_cutout(*args)
        return _trimap_engine(_torch_device()).outline(*args)


class SDMatteTemporalSmooth:
    """Frames + their alphas -> the alphas filtered along time on the GPU: the batch is a clip.  A neighbouring frame contributes to a pixel only where the
    picture around it did not change between the two frames, so static regions stop shimmering while motion and cuts keep their own alpha.  One kernel
    launch, no optical flow.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE", {"tooltip": "the frames of the clip, in order (the batch axis is time)"}),
                             "alpha": ("MASK", {"tooltip": "the alpha matte of every frame"})},
                "optional": {"radius": ("INT", {"default": 2, "min": 1, "max": 4, "tooltip": "frames on either side that may contribute"}),
                             "patch": ("INT", {"default": 1, "min": 0, "max": 2,
                                               "tooltip": "the picture is compared over a (2 patch + 1)^2 neighbourhood of the pixel"}),
                             "color_tolerance": ("FLOAT", {"default": 0.1, "min": 0.001, "max": 1.0, "step": 0.005,
                                                           "tooltip": "RMS colour change at which a neighbouring frame stops contributing"}),
                             "strength": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.05, "tooltip": "0 returns the alpha unchanged"}),
                             "max_change": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01,
                                                      "tooltip": "the most a pixel's alpha may move away from its own frame's value"}),
                             "clip_len": ("INT", {"default": 0, "min": 0, "max": 1 << 20,
                                                  "tooltip": "0: the batch is one clip; otherwise independent clips of this many frames"}),
                             "force_cpu": ("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU call"})}}

    RETURN_TYPES = ("MASK", )
    RETURN_NAMES = ("alpha", )
    FUNCTION = "smooth"
    CATEGORY = "Matting/SDMatte"

    def smooth(self, image, alpha, radius=2, patch=1, color_tolerance=0.1, strength=1.0, max_change=1.0, clip_len=0, force_cpu=False):
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if alpha.dim() == 2:
            alpha = alpha.unsqueeze(0)
        if tuple(alpha.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] alpha must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
        args = (image.detach().cpu(), alpha.detach().cpu(), int(radius), int(patch), float(color_tolerance), float(strength), float(max_change),
                int(clip_len))
        if force_cpu:      # an explicit request, never a silent substitute: the same function in torch
            return (temporal_smooth_alpha(*args), )
        return (_trimap_engine(_torch_device()).smooth_alpha_temporal(*args), )


class SDMatteTemporalSmoothMotion:
    """Frames + their alphas -> the alphas filtered along time AND along the motion on the GPU: the batch is a clip.  Every pixel looks for the patch around
    it in the neighbouring frames (integer displacements up to `search`) and is averaged with the alpha found there, so the soft edge and the hair of a
    moving subject stop shimmering too; cuts still keep their own alpha.  One kernel launch, no optical flow.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE", {"tooltip": "the frames of the clip, in order (the batch axis is time)"}),
                             "alpha": ("MASK", {"tooltip": "the alpha matte of every frame"})},
                "optional": {"radius": ("INT", {"default": 2, "min": 1, "max": 4, "tooltip": "frames on either side that may contribute"}),
                             "patch": ("INT", {"default": 1, "min": 0, "max": 2,
                                               "tooltip": "the picture is compared over a (2 patch + 1)^2 neighbourhood of the pixel"}),
                             "search": ("INT", {"default": 4, "min": 0, "max": 8,
                                                "tooltip": "the largest displacement, in pixels per frame step, that is looked for (0: no motion search)"}),
                             "color_tolerance": ("FLOAT", {"default": 0.1, "min": 0.001, "max": 1.0, "step": 0.005,
                                                           "tooltip": "RMS colour change at which a neighbouring frame stops contributing"}),
                             "motion_penalty": ("FLOAT", {"default": 0.02, "min": 0.0, "max": 1.0, "step": 0.005,
                                                          "tooltip": "what a squared pixel of displacement costs, in units of color_tolerance squared"}),
                             "strength": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.05, "tooltip": "0 returns the alpha unchanged"}),
                             "max_change": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01,
                                                      "tooltip": "the most a pixel's alpha may move away from its own frame's value"}),
                             "clip_len": ("INT", {"default": 0, "min": 0, "max": 1 << 20,
                                                  "tooltip": "0: the batch is one clip; otherwise independent clips of this many frames"}),
                             "force_cpu": ("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU call"})}}

    RETURN_TYPES = ("MASK", )
    RETURN_NAMES = ("alpha", )
    FUNCTION = "smooth"
    CATEGORY = "Matting/SDMatte"

    def smooth(self, image, alpha, radius=2, patch=1, search=4, color_tolerance=0.1, motion_penalty=0.02, strength=1.0, max_change=1.0, clip_len=0,
               force_cpu=False):
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if alpha.dim() == 2:
            alpha = alpha.unsqueeze(0)
        if tuple(alpha.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] alpha must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
        args = (image.detach().cpu(), alpha.detach().cpu(), int(radius), int(patch), int(search), float(color_tolerance), float(motion_penalty),
                float(strength), float(max_change), int(clip_len))
        if force_cpu:      # an explicit request, never a silent substitute: the same function in torch
            return (temporal_smooth_alpha_motion(*args), )
        return (_trimap_engine(_torch_device()).smooth_alpha_motion(*args), )


class SDMatteDefocus:
    """Image + alpha -> the subject over its own background out of focus ("portrait mode", background blur) on the GPU.  The blur is a disc, as a lens's
    is, it is normalised and does not see the subject, so the subject's colours leave no halo around the silhouette; bright background points can be
    boosted into round highlights.  Two kernel launches.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE", {"tooltip": "the photo"}),
                             "alpha": ("MASK", {"tooltip": "alpha matte of the photo (alpha_mask of Apply SDMatte)"})},
                "optional": {"foreground": ("IMAGE", {"tooltip": "foreground colours (SDMatte Foreground Colours); default: the photo"}),
                             "background": ("IMAGE", {"tooltip": "background colours (SDMatte Foreground Colours); default: the photo"}),
                             "radius_px": ("INT", {"default": 16, "min": 1, "max": 64, "tooltip": "radius of the blur disc in pixels"}),
                             "highlight_gain": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 64.0, "step": 0.5,
                                                          "tooltip": "extra weight of background pixels per unit of brightness above the threshold"}),
                             "highlight_threshold": ("FLOAT", {"default": 0.8, "min": 0.0, "max": 1.0, "step": 0.01,
                                                               "tooltip": "brightness (mean of r, g, b) above which a pixel counts as a highlight"}),
                             "decontaminate": ("BOOLEAN", {"default": False,
                                                           "tooltip": "with neither foreground nor background connected: estimate both from the photo first"}),
                             "force_cpu": ("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU call"})}}

    RETURN_TYPES = ("IMAGE", )
    RETURN_NAMES = ("image", )
    FUNCTION = "defocus"
    CATEGORY = "Matting/SDMatte"

    def defocus(self, image, alpha, foreground=None, background=None, radius_px=16, highlight_gain=0.0, highlight_threshold=0.8, decontaminate=False,
                force_cpu=False):
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if alpha.dim() == 2:
            alpha = alpha.unsqueeze(0)
        if tuple(alpha.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] alpha must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
        for name, t in (("foreground", foreground), ("background", background)):
            if t is not None and tuple(t.shape) != tuple(image.shape):
                raise ValueError(f"[SDMatte] {name} must be [B,H,W,3] of the image {tuple(image.shape)}, got {tuple(t.shape)}")
        params = (int(radius_px), float(highlight_gain), float(highlight_threshold))
        estimate = bool(decontaminate) and foreground is None and background is None
        if force_cpu:      # an explicit request, never a silent substitute: the same functions in torch
            image, alpha = image.detach().cpu(), alpha.detach().cpu()
            fg = foreground.detach().cpu() if foreground is not None else None
            bg = background.detach().cpu() if background is not None else None
            if estimate:
                fg, bg, _ = estimate_foreground(image, alpha)
            return (defocus_background(image, alpha, fg, bg, *params), )
        device = _torch_device()
        eng = _trimap_engine(device)
        image, alpha = image.detach().to(device), alpha.detach().to(device)
        fg = foreground.detach().to(device) if foreground is not None else None
        bg = background.detach().to(device) if background is not None else None
        if estimate:       # both planes stay on the device: the two calls are ordered on torch's current stream
            fg, bg = eng.estimate_foreground(image, alpha, sync=False)
        return (eng.defocus_background(image, alpha, fg, bg, *params, sync=False).cpu(), )


class SDMatteCleanPlate:
    """Image + alpha -> the photo without its subject (the "clean plate"): the hole is filled by push-pull from the background around it, the background
    itself comes back bit for bit, and the subject's colour never enters.  For moving the subject inside its own photo, a two-layer parallax split, a
    background for the defocus / harmonize nodes, or the pre-fill in front of an inpainting model.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE", {"tooltip": "the photo"}),
                             "alpha": ("MASK", {"tooltip": "alpha matte of the photo (alpha_mask of Apply SDMatte)"})},
                "optional": {"hole": ("MASK", {"tooltip": "more to take out (a shadow, a second object): combined with the alpha by max"}),
                             "background": ("IMAGE", {"tooltip": "background colours (SDMatte Foreground Colours); default: the photo"}),
                             "alpha_cut": ("FLOAT", {"default": 0.0625, "min": 2.0 ** -10, "max": 1.0, "step": 0.0001,
                                                     "tooltip": "pixels count as background with the weight 1 - alpha / alpha_cut; 1 with clean background "
                                                                "colours, small without"}),
                             "decontaminate": ("BOOLEAN", {"default": False,
                                                           "tooltip": "with no background connected: estimate the background colours from the photo first"}),
                             "force_cpu": ("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU call"})}}

    RETURN_TYPES = ("IMAGE", )
    RETURN_NAMES = ("plate", )
    FUNCTION = "fill"
    CATEGORY = "Matting/SDMatte"

    def fill(self, image, alpha, hole=None, background=None, alpha_cut=0.0625, decontaminate=False, force_cpu=False):
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        if alpha.dim() == 2:
            alpha = alpha.unsqueeze(0)
        if tuple(alpha.shape) != tuple(image.shape[:3]):
            raise ValueError(f"[SDMatte] alpha must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(alpha.shape)}")
        if hole is not None:
            if hole.dim() == 2:
                hole = hole.unsqueeze(0)
            if tuple(hole.shape) != tuple(image.shape[:3]):
                raise ValueError(f"[SDMatte] hole must be [B,H,W] of the image {tuple(image.shape[:3])}, got {tuple(hole.shape)}")
        if background is not None and tuple(background.shape) != tuple(image.shape):
            raise ValueError(f"[SDMatte] background must be [B,H,W,3] of the image {tuple(image.shape)}, got {tuple(background.shape)}")
        alpha_cut = float(alpha_cut)
        estimate = bool(decontaminate) and background is None
        if force_cpu:      # an explicit request, never a silent substitute: the same functions in torch
            image, alpha = image.detach().cpu(), alpha.detach().cpu()
            hole = hole.detach().cpu() if hole is not None else None
            bg = background.detach().cpu() if background is not None else None
            if estimate:
                _, bg, _ = estimate_foreground(image, alpha)
            return (clean_plate(image, alpha, bg, hole, alpha_cut), )
        device = _torch_device()
        eng = _trimap_engine(device)
        image, alpha = image.detach().to(device), alpha.detach().to(device)
        hole = hole.detach().to(device) if hole is not None else None
        bg = background.detach().to(device) if background is not None else None
        if estimate:       # the plane stays on the device: the two calls are ordered on torch's current stream
            _, bg = eng.estimate_foreground(image, alpha, sync=False)
        return (eng.fill_background(image, alpha, bg, hole, alpha_cut, sync=False).cpu(), )


class SDMatteHarmonize:
    """Foreground + alpha + a new background -> the cut-out sitting in that scene on the GPU: its colours matched to the scene's light (mean and spread of
    brightness and of the two colour axes), the scene's light wrapped around its edge, then composed.  One to four kernel launches.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        unit = lambda d, tip: ("FLOAT", {"default": d, "min": 0.0, "max": 1.0, "step": 0.05, "tooltip": tip})
        return {"required": {"foreground": ("IMAGE", {"tooltip": "foreground colours of the cut-out (foreground of SDMatte Foreground Colours, or the image)"}),
                             "alpha": ("MASK", {"tooltip": "alpha matte of the foreground"}),
                             "background": ("IMAGE", {"tooltip": "the new scene (one image, or one per foreground); another size is scaled to cover and centre-cropped"})},
                "optional": {"luma_strength": unit(0.6, "how far the subject's brightness moves to the scene's (0 = not at all)"),
                             "chroma_strength": unit(0.8, "how far the subject's colour cast moves to the scene's"),
                             "contrast_strength": unit(0.5, "how far the spread of brightness and colour follows the scene's"),
                             "wrap_strength": unit(0.5, "how much of the scene's light spills over the subject's edge (0 = no light wrap)"),
                             "wrap_sigma": ("FLOAT", {"default": 6.0, "min": 0.1, "max": 16.0, "step": 0.1, "tooltip": "reach of the light wrap in pixels (Gaussian sigma)"}),
                             "force_cpu": ("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU call"})}}

    RETURN_TYPES = ("IMAGE", "IMAGE")
    RETURN_NAMES = ("image", "foreground")
    FUNCTION = "harmonize"
    CATEGORY = "Matting/SDMatte"

    def harmonize(self, foreground, alpha, background, luma_strength=0.6, chroma_strength=0.8, contrast_strength=0.5, wrap_strength=0.5, wrap_sigma=6.0,
                  force_cpu=False):
        if foreground.dim() != 4 or foreground.shape[-1] != 3:
            raise ValueError(f"[SDMatte] foreground must be [B,H,W,3], got {tuple(foreground.shape)}")
        if alpha.dim() == 2:
            alpha = alpha.unsqueeze(0)
        if tuple(alpha.shape) != tuple(foreground.shape[:3]):
            raise ValueError(f"[SDMatte] alpha must be [B,H,W] of the foreground {tuple(foreground.shape[:3])}, got {tuple(alpha.shape)}")
        B, H, W = (int(v) for v in foreground.shape[:3])
        if background.dim() != 4 or background.shape[-1] != 3 or int(background.shape[0]) not in (1, B):
            raise ValueError(f"[SDMatte] background must be [1 or {B},h,w,3], got {tuple(background.shape)}")
        params = (float(luma_strength), float(chroma_strength), float(contrast_strength), float(wrap_strength), float(wrap_sigma))
        bg = fit_background(background.detach().cpu(), H, W)
        if force_cpu:      # an explicit request, never a silent substitute: the same function in torch
            return harmonize_cutout(foreground.detach().cpu(), alpha.detach().cpu(), bg, *params, return_fg=True)
        device = _torch_device()
        out, fg_out = _trimap_engine(device).harmonize(foreground.detach().to(device), alpha.detach().to(device), bg.to(device), *params, return_fg=True,
                                                       sync=False)
        return (out.cpu(), fg_out.cpu())


_KEY_INPUTS = {
    "clip_fg": ("FLOAT", {"default": 0.15, "min": 0.0, "max": 0.99, "step": 0.01,
                          "tooltip": "screen excess (as a share of the screen's own) at and below which a pixel is all subject"}),
    "clip_bg": ("FLOAT", {"default": 0.85, "min": 0.01, "max": 1.0, "step": 0.01, "tooltip": "screen excess at and above which a pixel is all screen"}),
    "sure_fg": ("FLOAT", {"default": 0.05, "min": -1.0, "max": 1.0, "step": 0.01,
                          "tooltip": "the trimap calls a pixel certain subject only with a screen excess up to this"}),
    "sure_bg": ("FLOAT", {"default": 0.95, "min": -1.0, "max": 2.0, "step": 0.01,
                          "tooltip": "the trimap calls a pixel certain screen only with a screen excess of at least this"}),
    "erode_px": ("INT", {"default": 10, "min": 0, "max": 255, "tooltip": "unknown band inside the key's 0.5 contour, in pixels"}),
    "dilate_px": ("INT", {"default": 10, "min": 0, "max": 255, "tooltip": "unknown band outside the key's 0.5 contour, in pixels"}),
    "despill": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.05, "tooltip": "how much of the screen's excess is taken out of the image"}),
}


class SDMatteChromaKey:
    """A green- or blue-screen shot -> the trimap for Apply SDMatte, the classical key, the despilled image and the screen, on the GPU.  The screen's
    colour is found in the image (or the batch, for a clip); with screen_correction the key is made a second time against the screen's colour at each
    pixel (the clean plate of the first key), so uneven lighting and shadows on the screen key out.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE", {"tooltip": "the shot in front of the screen"})},
                "optional": dict({"hint": (["green", "blue", "any"], {"default": "green", "tooltip": "which saturated colour counts as a screen"}),
                                  "share": ("BOOLEAN", {"default": False, "tooltip": "one screen colour for the whole batch (a clip)"}),
                                  "screen_correction": ("BOOLEAN", {"default": True,
                                                                    "tooltip": "key against the screen's colour at each pixel (the clean plate of a first key)"}),
                                  "screen_cut": ("FLOAT", {"default": 0.25, "min": 2.0 ** -10, "max": 1.0, "step": 0.01,
                                                           "tooltip": "first-key value from which a pixel no longer counts as screen for the plate"})},
                                 **_KEY_INPUTS,
                                 force_cpu=("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU calls"}))}

    RETURN_TYPES = ("MASK", "MASK", "IMAGE", "IMAGE")
    RETURN_NAMES = ("trimap", "key", "despilled", "screen")
    FUNCTION = "key"
    CATEGORY = "Matting/SDMatte"

    def key(self, image, hint="green", share=False, screen_correction=True, screen_cut=0.25, clip_fg=0.15, clip_bg=0.85, sure_fg=0.05, sure_bg=0.95,
            erode_px=10, dilate_px=10, despill=1.0, force_cpu=False):
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        args = (hint, bool(share), bool(screen_correction), float(screen_cut), float(clip_fg), float(clip_bg), float(sure_fg), float(sure_bg),
                int(erode_px), int(dilate_px), float(despill), ("trimap", "key", "despilled"))
        if force_cpu:      # an explicit request, never a silent substitute: the same functions in torch
            trimap, key, despilled, screen = key_screen(image.detach().cpu(), *args)
        else:
            device = _torch_device()
            trimap, key, despilled, screen = (t.cpu() for t in _trimap_engine(device).key_screen(image.detach().to(device), *args, sync=False))
        return (trimap, key, despilled, screen if screen.dim() == 4 else screen.view(-1, 1, 1, 3))


class SDMatteDespill:
    """An image (or the foreground colours of SDMatte Foreground Colours) + the screen of SDMatte Chroma Key -> the image without the screen's
    reflected light: the excess of the screen's channel over the larger of the other two is taken out.  One kernel launch.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE", {"tooltip": "the shot, or foreground colours estimated from it"}),
                             "screen": ("IMAGE", {"tooltip": "the screen of SDMatte Chroma Key: one colour per image [B,1,1,3], or a colour per pixel"})},
                "optional": {"despill": _KEY_INPUTS["despill"],
                             "force_cpu": ("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU call"})}}

    RETURN_TYPES = ("IMAGE", )
    RETURN_NAMES = ("image", )
    FUNCTION = "despill"
    CATEGORY = "Matting/SDMatte"

    def despill(self, image, screen, despill=1.0, force_cpu=False):
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"[SDMatte] image must be [B,H,W,3], got {tuple(image.shape)}")
        B, H, W = (int(v) for v in image.shape[:3])
        if screen.dim() != 4 or tuple(screen.shape) not in ((B, 1, 1, 3), (B, H, W, 3)):
            raise ValueError(f"[SDMatte] screen must be [B,1,1,3] or [B,H,W,3] of the image {(B, H, W)}, got {tuple(screen.shape)}")
        if force_cpu:      # an explicit request, never a silent substitute: the same function in torch
            return (chroma_key(image.detach().cpu(), screen.detach().cpu(), despill=float(despill), want=("despilled", )), )
        device = _torch_device()
        out = _trimap_engine(device).chroma_key(image.detach().to(device), screen.detach().to(device), despill=float(despill), want=("despilled", ),
                                                sync=False)
        return (out.cpu(), )


class SDMatteMetrics:
    """Alpha + ground truth (+ trimap) -> the matting literature's SAD, MSE, Grad and Conn over the trimap's unknown band (the whole frame without a
    trimap), on the GPU: 2 kernel launches, 63 with connectivity.  Needs no checkpoint."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"alpha": ("MASK", {"tooltip": "the alpha matte to score"}),
                             "ground_truth": ("MASK", {"tooltip": "the reference alpha"})},
                "optional": {"trimap": ("MASK", {"tooltip": "the trimap: only its unknown band (values near 0.5) is scored; without it the whole frame"}),
                             "grad_sigma": ("FLOAT", {"default": 1.4, "min": 0.25, "max": 4.0, "step": 0.05, "tooltip": "sigma of the Grad metric's Gaussian derivative"}),
                             "connectivity": ("BOOLEAN", {"default": True, "tooltip": "also compute Conn (ten labellings per image)"}),
                             "force_cpu": ("BOOLEAN", {"default": False, "tooltip": "evaluate the torch restatement on the CPU instead of the GPU call"})}}

    RETURN_TYPES = ("STRING", "FLOAT", "FLOAT", "FLOAT", "FLOAT")
    RETURN_NAMES = ("report", "sad", "mse", "grad", "conn")
    FUNCTION = "score"
    CATEGORY = "Matting/SDMatte"
    OUTPUT_NODE = True

    def score(self, alpha, ground_truth, trimap=None, grad_sigma=1.4, connectivity=True, force_cpu=False):
        planes = [alpha, ground_truth] + ([trimap] if trimap is not None else [])
        planes = [t.unsqueeze(0) if t.dim() == 2 else t for t in planes]
        if any(t.dim() != 3 or tuple(t.shape) != tuple(planes[0].shape) for t in planes):
            raise ValueError(f"[SDMatte] alpha, ground truth and trimap must be equal [B,H,W], got {[tuple(t.shape) for t in planes]}")
        if force_cpu:      # an explicit request, never a silent substitute: the same function in torch
            res = matte_metrics(*(t.detach().cpu().float() for t in planes), grad_sigma=float(grad_sigma), conn=bool(connectivity))
        else:
            device = _torch_device()
            res = _trimap_engine(device).matte_metrics(*(t.detach().to(device) for t in planes), grad_sigma=float(grad_sigma), conn=bool(connectivity))
            res = {k: v.cpu() for k, v in res.items()}
        text, means = metrics_report(res)
        return (text, ) + means


def node_mappings(extra: bool, foreground: bool = False, refine: bool = False, clean: bool = False, roi: bool = False, canvas: bool = False,
                  subjects: bool = False, edge: bool = False, video: bool = False, motion: bool = False, defocus: bool = False):
    """(NODE_CLASS_MAPPINGS, NODE_DISPLAY_NAME_MAPPINGS): the reference's surface, plus the two mask nodes when `extra`, plus the foreground
    node when `foreground`, plus the alpha refinement node when `refine`, plus the mask clean-up node when `clean`, plus the subject-box node when `roi`,
    plus the canvas node when `canvas`, plus the box-per-subject node when `subjects`, plus the two
    distance-field nodes (mask offset, outline) when `edge`, plus the temporal smoothing node when `video`, plus the motion-compensated one when `motion`,
    plus the background defocus node when `defocus`.  (The harmonize node is added by `with_harmonize_node`.)"""
    classes = {"SDMatteApply": SDMatteApply}
    names = {"SDMatteApply": "Apply SDMatte"}
    if extra:
        classes.update({"SDMatteTrimapFromMask": SDMatteTrimapFromMask, "SDMatteApplyMask": SDMatteApplyMask})
        names.update({"SDMatteTrimapFromMask": "SDMatte Trimap From Mask", "SDMatteApplyMask": "Apply SDMatte (Mask)"})
    if foreground:
        classes["SDMatteForeground"] = SDMatteForeground
        names["SDMatteForeground"] = "SDMatte Foreground Colours"
    if refine:
        classes["SDMatteRefineAlpha"] = SDMatteRefineAlpha
        names["SDMatteRefineAlpha"] = "SDMatte Refine Alpha"
    if clean:
        classes["SDMatteCleanMask"] = SDMatteCleanMask
        names["SDMatteCleanMask"] = "SDMatte Clean Mask"
    if roi:
        classes["SDMatteApplyROI"] = SDMatteApplyROI
        names["SDMatteApplyROI"] = "Apply SDMatte (Subject Box)"
    if canvas:
        classes["SDMatteCanvas"] = SDMatteCanvas
        names["SDMatteCanvas"] = "SDMatte Canvas"
    if subjects:
        classes["SDMatteApplySubjects"] = SDMatteApplySubjects
        names["SDMatteApplySubjects"] = "Apply SDMatte (Subjects)"
    if edge:
        classes.update({"SDMatteOffsetMask": SDMatteOffsetMask, "SDMatteOutline": SDMatteOutline})
        names.update({"SDMatteOffsetMask": "SDMatte Grow / Shrink Mask", "SDMatteOutline": "SDMatte Outline"})
    if video:
        classes["SDMatteTemporalSmooth"] = SDMatteTemporalSmooth
        names["SDMatteTemporalSmooth"] = "SDMatte Temporal Smooth"
    if motion:
        classes["SDMatteTemporalSmoothMotion"] = SDMatteTemporalSmoothMotion
        names["SDMatteTemporalSmoothMotion"] = "SDMatte Temporal Smooth (Motion)"
    if defocus:
        classes["SDMatteDefocus"] = SDMatteDefocus
        names["SDMatteDefocus"] = "SDMatte Defocus Background"
    return classes, names


def with_harmonize_node(mappings, harmonize: bool = True):
    """(classes, names) of `node_mappings` plus `SDMatteHarmonize` when `harmonize`; the argument is not modified.  A function of its own: the argument
    list of `node_mappings` is pinned by its callers."""
    classes, names = dict(mappings[0]), dict(mappings[1])
    if harmonize:
        classes["SDMatteHarmonize"] = SDMatteHarmonize
        names["SDMatteHarmonize"] = "SDMatte Harmonize"
    return classes, names


def with_metrics_node(mappings, metrics: bool = True):
    """(classes, names) of `mappings` plus `SDMatteMetrics` when `metrics`; the argument is not modified (as `with_harmonize_node`)."""
    classes, names = dict(mappings[0]), dict(mappings[1])
    if metrics:
        classes["SDMatteMetrics"] = SDMatteMetrics
        names["SDMatteMetrics"] = "SDMatte Metrics (SAD / MSE / Grad / Conn)"
    return classes, names


def with_tiled_node(mappings, tiled: bool = True):
    """(classes, names) of `mappings` plus `SDMatteApplyTiled` when `tiled`; the argument is not modified (as `with_harmonize_node`)."""
    classes, names = dict(mappings[0]), dict(mappings[1])
    if tiled:
        classes["SDMatteApplyTiled"] = SDMatteApplyTiled
        names["SDMatteApplyTiled"] = "Apply SDMatte (Tiled)"
    return classes, names


def with_plate_node(mappings, plate: bool = True):
    """(classes, names) of `mappings` plus `SDMatteCleanPlate` when `plate`; the argument is not modified (as `with_harmonize_node`)."""
    classes, names = dict(mappings[0]), dict(mappings[1])
    if plate:
        classes["SDMatteCleanPlate"] = SDMatteCleanPlate
        names["SDMatteCleanPlate"] = "SDMatte Clean Plate (Fill Background)"
    return classes, names


def with_key_nodes(mappings, on: bool = True):
    """(classes, names) of `mappings` plus `SDMatteChromaKey` and `SDMatteDespill` when `on`; the argument is not modified (as `with_harmonize_node`)."""
    classes, names = dict(mappings[0]), dict(mappings[1])
    if on:
        classes["SDMatteChromaKey"] = SDMatteChromaKey
        names["SDMatteChromaKey"] = "SDMatte Chroma Key (Green Screen)"
        classes["SDMatteDespill"] = SDMatteDespill
        names["SDMatteDespill"] = "SDMatte Despill"
    return classes, names


# the nodes beyond the reference are opt-in (SDMATTE_EXTRA_NODES=1, SDMATTE_FOREGROUND_NODE=1, SDMATTE_REFINE_NODE=1, SDMATTE_CLEAN_NODE=1, SDMATTE_ROI_NODE=1, SDMATTE_CANVAS_NODE=1, SDMATTE_SUBJECTS_NODE=1, SDMATTE_EDGE_NODES=1, SDMATTE_VIDEO_NODE=1, SDMATTE_MOTION_NODE=1, SDMATTE_DEFOCUS_NODE=1, SDMATTE_HARMONIZE_NODE=1, SDMATTE_METRICS_NODE=1, SDMATTE_TILED_NODE=1, SDMATTE_PLATE_NODE=1, SDMATTE_KEY_NODES=1), like the multi-GPU fan-out
# (SDMATTE_MULTI_GPU)
NODE_CLASS_MAPPINGS, NODE_DISPLAY_NAME_MAPPINGS = with_key_nodes(with_plate_node(with_tiled_node(with_metrics_node(with_harmonize_node(node_mappings(os.environ.get("SDMATTE_EXTRA_NODES") == "1",
                                                                os.environ.get("SDMATTE_FOREGROUND_NODE") == "1",
                                                                os.environ.get("SDMATTE_REFINE_NODE") == "1",
                                                                os.environ.get("SDMATTE_CLEAN_NODE") == "1",
                                                                os.environ.get("SDMATTE_ROI_NODE") == "1",
                                                                os.environ.get("SDMATTE_CANVAS_NODE") == "1",
                                                                os.environ.get("SDMATTE_SUBJECTS_NODE") == "1",
                                                                os.environ.get("SDMATTE_EDGE_NODES") == "1",
                                                                os.environ.get("SDMATTE_VIDEO_NODE") == "1",
                                                                os.environ.get("SDMATTE_MOTION_NODE") == "1",
                                                                os.environ.get("SDMATTE_DEFOCUS_NODE") == "1"),
                                                                      os.environ.get("SDMATTE_HARMONIZE_NODE") == "1"),
                                                                      os.environ.get("SDMATTE_METRICS_NODE") == "1"),
                                                                      os.environ.get("SDMATTE_TILED_NODE") == "1"),
                                                                      os.environ.get("SDMATTE_PLATE_NODE") == "1"),
                                                                      os.environ.get("SDMATTE_KEY_NODES") == "1")
