"""The slice of the `clip` package surface that UniIR uses (clip.load, clip.tokenize), backed by uniir_amd.

Reference call sites: src/models/uniir_clip/clip_scorefusion/clip_sf.py:25-26 (clip.load -> (model, preprocess);
clip.tokenize).  Upstream downloads weights / ships a BPE vocabulary; neither exists offline, so:
  * load(): builds the architecture for `name` (random init, upstream std choices) and, when
    <download_root>/<name>.pt (a state dict, or a checkpoint with a "state_dict"/"model" entry) exists, loads it;
  * tokenize(): the byte-level BPE of clip/simple_tokenizer.py (BPETokenizer below, pinned on a synthetic merge list
    against an independent implementation: tests/golden/g15_bpe.json); it needs OpenAI's bpe_simple_vocab_16e6.txt.gz
    at $UNIIR_BPE_PATH, $UNIIR_CLIP_ROOT or ~/.cache/clip and raises without it (parity on the REAL vocabulary is
    unpinned offline, SURVEY.md section 7 'No network').
"""
import os

import numpy as np
import torch

from .clip_model import CLIP, CLIP_CONFIGS

_MEAN = (0.48145466, 0.4578275, 0.40821073)
_STD = (0.26862954, 0.26130258, 0.27577711)


def _preprocess(n_px):
    def fn(image):
        """PIL image -> float tensor [3, n_px, n_px]: bicubic resize of the short side, centre crop, RGB,
        CLIP mean/std normalisation (upstream clip._transform)."""
        from PIL import Image
        w, h = image.size
        nh, nw, top, left = resize_geometry(h, w, n_px)          # torchvision Resize + CenterCrop integers
        image = image.resize((nw, nh), Image.BICUBIC)
        image = image.crop((left, top, left + n_px, top + n_px)).convert("RGB")
        a = torch.from_numpy(np.asarray(image, dtype=np.float32) / 255.0).permute(2, 0, 1)
        return (a - torch.tensor(_MEAN).view(3, 1, 1)) / torch.tensor(_STD).view(3, 1, 1)

    return fn


def resize_geometry(h, w, n_px, center_crop=True):
    """integer geometry of the transform: torchvision Resize(n_px) (short side n_px, long side int(n_px * long / short)) +
    CenterCrop (offsets round-half-even((size - n_px) / 2)) as upstream clip._transform composes them; center_crop=False
    is BLIP's square Resize((n_px, n_px)) (blip_transform.py:41-48).  -> (oh, ow, top, left)"""
    if not center_crop:
        return n_px, n_px, 0, 0
    if w <= h:
        ow, oh = n_px, int(n_px * h / w)
    else:
        oh, ow = n_px, int(n_px * w / h)
    return oh, ow, int(round((oh - n_px) / 2.0)), int(round((ow - n_px) / 2.0))


def preprocess_on_device(images, n_px, device, mean=_MEAN, std=_STD, center_crop=True, out=None):
    """Decoded RGB images (PIL images or uint8 [h, w, 3] arrays / tensors, any sizes) -> fp32 [M, 3, n_px, n_px] on the
    device through libuniir_hip's uniir_image_preprocess: the resize / crop / normalise chain of the reference's CPU
    workers, bit-exact with Pillow's BICUBIC for the integer stage (include/uniir_hip.h [IMAGE])."""
    import ctypes

    from . import _lib, ops
    lib = _lib.load()
    M = len(images)
    if out is None:
        out = torch.empty(M, 3, n_px, n_px, device=device, dtype=torch.float32)
    mean_c, std_c = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    stream = torch.cuda.current_stream(device).cuda_stream
    ws = None
    for i, img in enumerate(images):
        if not isinstance(img, (torch.Tensor, np.ndarray)):
            img = np.asarray(img.convert("RGB"), dtype=np.uint8)
        t = torch.as_tensor(img)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("images must be RGB uint8 [h, w, 3]")
        t = t.contiguous().to(device, non_blocking=True)
        h, w = int(t.shape[0]), int(t.shape[1])
        oh, ow, top, left = resize_geometry(h, w, n_px, center_crop)
        need = lib.uniir_image_workspace_bytes(h, w, oh, ow, n_px)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, device=device, dtype=torch.uint8)
        ops.check(lib.uniir_image_preprocess(t.data_ptr(), h, w, oh, ow, top, left, n_px, mean_c, std_c, out[i].data_ptr(),
                                             ws.data_ptr(), ws.numel(), stream), "image_preprocess")
    return out


class PackedImages:
    """A batch of decoded images ready for ONE host -> device copy and ONE call of uniir_image_preprocess_batch: a single
    uint8 host buffer holding [descriptor table | plan table | pixels, every image 16-byte aligned] (include/uniir_hip.h
    [IMAGE]).  `geoms[i]` = (box_left, box_top, box_w, box_h, oh, ow, top, left, flip) of image i, or None for the CLIP
    chain on the whole image; `out_index[i]` = the output slot it lands in (default i).  The plan call validates the table
    on the host: a malformed descriptor raises here, before anything reaches the device.  `augs[i]` = the augmentation ops of
    image i as (name | op code, arg) pairs (uniir_amd/randaugment.py) or None; with `augs` the aug table of
    uniir_image_aug_plan joins the same buffer, after the plan table, and run() calls the _aug entry point."""

    def __init__(self, images, geoms, n_px, out_index=None, out_items=None, pin=False, augs=None):
        import ctypes

        from . import _lib
        lib = _lib.load()
        count = len(images)
        geoms = [None] * count if geoms is None else list(geoms)
        out_index = list(range(count)) if out_index is None else [int(i) for i in out_index]
        if len(geoms) != count or len(out_index) != count:
            raise ValueError("images, geoms and out_index must have one entry per image")
        self.count, self.n_px = count, int(n_px)
        self.out_items = int(out_items) if out_items is not None else (max(out_index) + 1 if out_index else 0)
        arrays, descs, off = [], (_lib.ImageDesc * max(count, 1))(), 0
        for i, img in enumerate(images):
            if isinstance(img, torch.Tensor):
                if img.is_cuda:
                    raise ValueError("PackedImages packs host images")
                a = img.contiguous().numpy()
            elif isinstance(img, np.ndarray):
                a = np.ascontiguousarray(img)
            else:
                a = np.asarray(img.convert("RGB"), dtype=np.uint8)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("images must be RGB uint8 [h, w, 3]")
            h, w = int(a.shape[0]), int(a.shape[1])
            g = geoms[i]
            if g is None:
                oh, ow, top, left = resize_geometry(h, w, n_px)
                g = (0, 0, w, h, oh, ow, top, left, 0)
            d = descs[i]
            d.offset, d.h, d.w = off, h, w
            d.box_left, d.box_top, d.box_w, d.box_h, d.oh, d.ow, d.top, d.left, d.flip = (int(v) for v in g)
            d.out_index = out_index[i]
            arrays.append(a)
            off += (a.size + 15) & ~15
        plans, self.info = (_lib.ImagePlan * max(count, 1))(), _lib.ImageBatchInfo()
        _lib.check(lib.uniir_image_batch_plan(descs, count, self.n_px, max(self.out_items, 1), off, plans,
                                              ctypes.byref(self.info)), "image_batch_plan")
        nd, npl = count * ctypes.sizeof(_lib.ImageDesc), count * ctypes.sizeof(_lib.ImagePlan)
        self.plan0 = (nd + 255) & ~255
        self.pix0 = self.plan0 + ((npl + 255) & ~255)
        self.aug_info, aug_table = None, None
        if augs is not None and count:
            from . import randaugment
            if len(augs) != count:
                raise ValueError("augs must have one entry per image")
            codes, args, slots = randaugment.op_arrays(augs)
            aug_table, self.aug_info = (_lib.ImageAug * count)(), _lib.ImageAugInfo()
            _lib.check(lib.uniir_image_aug_plan(codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                args.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), count, slots, self.n_px,
                                                aug_table, ctypes.byref(self.aug_info)), "image_aug_plan")
            self.aug0, na = self.pix0, count * ctypes.sizeof(_lib.ImageAug)
            self.pix0 = self.aug0 + ((na + 255) & ~255)
        self.blob = torch.empty(self.pix0 + off, dtype=torch.uint8, pin_memory=bool(pin))
        self.pinned = bool(pin)
        view = self.blob.numpy()
        if count:
            view[:nd] = np.frombuffer(descs, dtype=np.uint8, count=nd)
            view[self.plan0:self.plan0 + npl] = np.frombuffer(plans, dtype=np.uint8, count=npl)
        if aug_table is not None:
            view[self.aug0:self.aug0 + na] = np.frombuffer(aug_table, dtype=np.uint8, count=na)
        for i, a in enumerate(arrays):
            view[self.pix0 + descs[i].offset:self.pix0 + descs[i].offset + a.size] = a.reshape(-1)
        self.descs, self.plans = descs, plans

    def run(self, device, mean=_MEAN, std=_STD, out=None, blob=None):
        """one non_blocking copy of the buffer (or `blob`: a device copy made earlier) + one call of the batched entry point
        on the current stream -> out fp32 [out_items, 3, n, n]; slots that no image names keep what they held"""
        import ctypes

        from . import _lib
        lib = _lib.load()
        n = self.n_px
        if out is None:
            out = torch.empty(self.out_items, 3, n, n, device=device, dtype=torch.float32)
        elif (tuple(out.shape) != (self.out_items, 3, n, n) or out.dtype != torch.float32 or not out.is_contiguous()
              or not out.is_cuda):
            raise ValueError(f"out must be a contiguous fp32 [{self.out_items}, 3, {n}, {n}] device tensor")
        if self.count == 0:
            return out
        dev = self.blob.to(device, non_blocking=True) if blob is None else blob
        need = int(self.info.workspace_bytes) + (int(self.aug_info.workspace_bytes) if self.aug_info is not None else 0)
        ws = torch.empty(max(need, 256), device=device, dtype=torch.uint8)
        mean_c, std_c = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        base = dev.data_ptr()
        if self.aug_info is not None:
            _lib.check(lib.uniir_image_preprocess_batch_aug(
                base + self.pix0, base, base + self.plan0, ctypes.byref(self.info), base + self.aug0, ctypes.byref(self.aug_info),
                mean_c, std_c, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(device).cuda_stream),
                "image_preprocess_batch_aug")
            return out
        _lib.check(lib.uniir_image_preprocess_batch(base + self.pix0, base, base + self.plan0, ctypes.byref(self.info), mean_c,
                                                    std_c, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    torch.cuda.current_stream(device).cuda_stream), "image_preprocess_batch")
        return out


def preprocess_batch_on_device(images, geoms, n_px, device, mean=_MEAN, std=_STD, out=None, out_index=None, pin=False):
    """The batched form of preprocess_on_device with per-image geometry (source box, resized size, window, flip: PackedImages):
    one packed host buffer, ONE non_blocking copy, ONE call of uniir_image_preprocess_batch (three launches whatever the
    batch size) -> fp32 [out_items, 3, n_px, n_px].  geoms=None is the CLIP chain on whole images, bit-identical to
    preprocess_on_device; `out_index` scatters into `out` (other slots untouched).  `images` may be a PackedImages built
    earlier (a pinned one by RawImageBatch.pin_memory)."""
    packed = images if isinstance(images, PackedImages) else PackedImages(
        images, geoms, n_px, out_index=out_index, out_items=None if out is None else int(out.shape[0]), pin=pin)
    return packed.run(device, mean, std, out=out)


def augment_batch_on_device(images, ops_per_image, out=None):
    """the augmentation op kernels alone (uniir_image_augment_batch): device uint8 [count, n, n, 3] + one list of (name | op code,
    arg) pairs per image (uniir_amd/randaugment.py; None = none) -> a new uint8 [count, n, n, 3]; two launches per op slot
    whatever the batch size.  -> (out, the plan's summary)"""
    import ctypes

    from . import _lib, randaugment
    lib = _lib.load()
    if (not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3
            or images.shape[1] != images.shape[2] or not images.is_contiguous()):
        raise ValueError("images must be a contiguous device uint8 [count, n, n, 3] tensor")
    count, n = int(images.shape[0]), int(images.shape[1])
    if len(ops_per_image) != count:
        raise ValueError("one op list per image")
    codes, args, slots = randaugment.op_arrays(ops_per_image)
    table, info = (_lib.ImageAug * max(count, 1))(), _lib.ImageAugInfo()
    _lib.check(lib.uniir_image_aug_plan(codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                        args.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), count, slots, n, table,
                                        ctypes.byref(info)), "image_aug_plan")
    if out is None:
        out = torch.empty_like(images)
    if count == 0:
        return out, info
    nbytes = count * ctypes.sizeof(_lib.ImageAug)
    dev_table = torch.from_numpy(np.frombuffer(table, dtype=np.uint8, count=nbytes).copy()).to(images.device)
    ws = torch.empty(max(int(info.workspace_bytes), 256), device=images.device, dtype=torch.uint8)
    _lib.check(lib.uniir_image_augment_batch(images.data_ptr(), dev_table.data_ptr(), ctypes.byref(info), out.data_ptr(),
                                             ws.data_ptr(), ws.numel(), torch.cuda.current_stream(images.device).cuda_stream),
               "image_augment_batch")
    return out, info


class RawImage:
    """a decoded RGB image waiting for the device transform (uint8 [h, w, 3], shareable between loader workers); `geom` =
    (box_left, box_top, box_w, box_h, flip) drawn by the worker (blip_front.RawBlipTransform), None = the whole image; `ops` =
    the augmentation ops it drew as (name, arg) pairs (uniir_amd/randaugment.py), None = none"""
    __slots__ = ("data", "geom", "ops")

    def __init__(self, data, geom=None, ops=None):
        self.data, self.geom, self.ops = data, geom, ops


class RawImageTransform:
    """Drop-in `img_preprocess_fn` that defers resize / crop / normalise to the GPU: the dataset worker only decodes, the
    collator builds a RawImageBatch, and the batch is transformed by `preprocess_batch_on_device` when it is moved to the
    device (host_utils.DevicePrefetcher / batch_to_device).  Bit-identical tensors to the CPU transform `_preprocess(n_px)`."""

    def __init__(self, n_px, mean=_MEAN, std=_STD, center_crop=True):
        self.n_px, self.mean, self.std, self.center_crop = n_px, tuple(mean), tuple(std), center_crop

    def __call__(self, image):
        return RawImage(torch.from_numpy(np.array(image.convert("RGB"), dtype=np.uint8)))


class RawImageBatch:
    """what a collator stacks instead of a float tensor when its items are RawImages (bare uint8 tensors are whole images;
    None = the black padding image of items without an image, which the reference builds as zeros AFTER normalisation)"""

    def __init__(self, images, transform):
        self.images, self.transform, self._packed = list(images), transform, None

    def size(self, dim=0):
        n = self.transform.n_px
        return (len(self.images), 3, n, n)[dim]

    def _pack(self, pin):
        t = self.transform
        have = [i for i, im in enumerate(self.images) if im is not None]
        datas, geoms, augs = [], [], []
        for i in have:
            im = self.images[i]
            data, g = (im.data, im.geom) if isinstance(im, RawImage) else (im, None)
            augs.append(im.ops if isinstance(im, RawImage) else None)     # a batch of Identity alone takes the plain entry: same bits
            left, top, bw, bh, flip = g if g is not None else (0, 0, int(data.shape[1]), int(data.shape[0]), 0)
            datas.append(data)      # the transform's own Resize (+ CenterCrop) applied to the box
            geoms.append((left, top, bw, bh) + resize_geometry(bh, bw, t.n_px, t.center_crop) + (flip,))
        return PackedImages(datas, geoms, t.n_px, out_index=have, out_items=len(self.images), pin=pin,
                            augs=augs if any(name not in ("Identity", 0) for a in augs if a for name, _ in a) else None)

    def pin_memory(self):
        if self._packed is None or not self._packed.pinned:
            self._packed = self._pack(pin=True)         # the single pinned buffer that to_device copies
        return self

    def to_device(self, device):
        t = self.transform
        out = torch.zeros(len(self.images), 3, t.n_px, t.n_px, device=device, dtype=torch.float32)
        packed = self._packed if self._packed is not None else self._pack(pin=False)
        return packed.run(device, t.mean, t.std, out=out)       # scattered to the positions that have an image


def load(name="ViT-B/32", device="cuda", jit=False, download_root=None, seed=0):
    if name not in CLIP_CONFIGS:
        raise RuntimeError(f"Model {name} not found; available models = {list(CLIP_CONFIGS)}")
    model = CLIP(CLIP_CONFIGS[name], seed=seed)
    if download_root:
        # the published file names: ViT-B-32.pt, ViT-L-14.pt, ViT-L-14-336px.pt
        path = os.path.join(os.path.expanduser(download_root), name.replace("/", "-").replace("@", "-") + ".pt")
        if os.path.exists(path):
            try:            # the published files are TorchScript archives (upstream clip.load falls back the other way)
                sd = torch.jit.load(path, map_location="cpu").state_dict()
            except RuntimeError:
                sd = torch.load(path, map_location="cpu", weights_only=False)
            sd = sd.get("state_dict", sd.get("model", sd)) if isinstance(sd, dict) else sd.state_dict()
            sd = {k: v.float() for k, v in sd.items() if k in model.state_dict()}
            model.load_state_dict(sd, strict=True)
        elif os.environ.get("UNIIR_ALLOW_RANDOM_INIT") != "1":
            # upstream clip.load downloads the file or fails; silently fine-tuning from random weights would produce
            # plausible-looking checkpoints and embeddings
            raise FileNotFoundError(f"pretrained CLIP weights not found: {path} (there is no network to download them from; "
                                    "put the openai/CLIP .pt file there, or set UNIIR_ALLOW_RANDOM_INIT=1 for a dry run)")
        else:
            import warnings
            warnings.warn(f"{path} is missing: CLIP {name} stays RANDOMLY INITIALISED (UNIIR_ALLOW_RANDOM_INIT=1)")
    if device is not None and str(device) != "cpu":
        model = model.to(device)
    return model, _preprocess(CLIP_CONFIGS[name]["image_resolution"])


class BPETokenizer:
    """Byte-level BPE of openai/CLIP (clip/simple_tokenizer.py, third-party: restated from its published behaviour, pinned
    in tests against transformers' CLIPTokenizer on a synthetic vocabulary -- the real 16e6 vocabulary is not available
    offline).  Vocabulary order: the 256 byte symbols, the same with the end-of-word marker, one entry per merge rule of
    the file (lines 1 .. 49152 - 256 - 2), then <|startoftext|>, <|endoftext|>."""
    EOW = "</w>"

    def __init__(self, bpe_path):
        import gzip
        import regex
        opener = gzip.open if bpe_path.endswith(".gz") else open
        with opener(bpe_path, "rt", encoding="utf-8") as f:
            lines = f.read().split("\n")
        rules = [tuple(ln.split()) for ln in lines[1:49152 - 256 - 2 + 1] if ln.strip()]
        # printable bytes stand for themselves, the other 68 get code points from 256 upwards (no whitespace / control symbols)
        keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
        self.byte_sym, extra = {}, 0
        for b in range(256):
            if b in keep:
                self.byte_sym[b] = chr(b)
            else:
                self.byte_sym[b] = chr(256 + extra)
                extra += 1
        base = [self.byte_sym[b] for b in keep] + [self.byte_sym[b] for b in range(256) if b not in keep]
        vocab = base + [v + self.EOW for v in base] + ["".join(r) for r in rules] + ["<|startoftext|>", "<|endoftext|>"]
        self.encoder = {tok: i for i, tok in enumerate(vocab)}
        self.rank = {r: i for i, r in enumerate(rules)}
        self.cache = {"<|startoftext|>": ("<|startoftext|>",), "<|endoftext|>": ("<|endoftext|>",)}
        self.splitter = regex.compile(
            r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+", regex.IGNORECASE)
        self.sot, self.eot = self.encoder["<|startoftext|>"], self.encoder["<|endoftext|>"]

    def _merge_word(self, token):
        if token in self.cache:
            return self.cache[token]
        parts = list(token[:-1]) + [token[-1] + self.EOW]
        while len(parts) > 1:
            best = min(((self.rank.get((a, b), float("inf")), i) for i, (a, b) in enumerate(zip(parts, parts[1:]))))
            if best[0] == float("inf"):
                break
            first, second = parts[best[1]], parts[best[1] + 1]
            merged, i = [], 0
            while i < len(parts):          # every occurrence of the best-ranked pair, left to right
                if i + 1 < len(parts) and parts[i] == first and parts[i + 1] == second:
                    merged.append(first + second)
                    i += 2
                else:
                    merged.append(parts[i])
                    i += 1
            parts = merged
        self.cache[token] = tuple(parts)
        return self.cache[token]

    @staticmethod
    def clean(text):
        import html
        import re
        try:
            import ftfy
            text = ftfy.fix_text(text)
        except ImportError:          # upstream repairs mojibake first; without ftfy well-formed text passes unchanged
            pass
        text = html.unescape(html.unescape(text)).strip()
        return re.sub(r"\s+", " ", text).strip().lower()

    def encode(self, text):
        ids = []
        for tok in self.splitter.findall(self.clean(text)):
            sym = "".join(self.byte_sym[b] for b in tok.encode("utf-8"))
            ids.extend(self.encoder[p] for p in self._merge_word(sym))
        return ids


_TOKENIZER = None


def _bpe_path():
    cands = [os.environ.get("UNIIR_BPE_PATH", "")]
    for root in (os.environ.get("UNIIR_CLIP_ROOT", ""), os.path.expanduser("~/.cache/clip")):
        cands.append(os.path.join(root, "bpe_simple_vocab_16e6.txt.gz"))
    for c in cands:
        if c and os.path.isdir(c):
            c = os.path.join(c, "bpe_simple_vocab_16e6.txt.gz")
        if c and os.path.isfile(c):
            return c
    return None


def tokenize(texts, context_length=77, truncate=False):
    """clip.tokenize: [SOT] + BPE ids + [EOT], zero padded to context_length -> int32 [n, context_length]; too long inputs
    raise unless truncate (then cut and the last id forced to EOT)."""
    global _TOKENIZER
    if _TOKENIZER is None:
        path = _bpe_path()
        if path is None:
            raise RuntimeError(
                "clip.tokenize needs OpenAI's bpe_simple_vocab_16e6.txt.gz, which is not available offline; set "
                "UNIIR_BPE_PATH to the file (or feed token ids: int32 [n, 77], SOT=49406 ... EOT=49407, zero padded)")
        _TOKENIZER = BPETokenizer(path)
    tk = _TOKENIZER
    if isinstance(texts, str):
        texts = [texts]
    out = torch.zeros(len(texts), context_length, dtype=torch.int32)
    for i, text in enumerate(texts):
        ids = [tk.sot] + tk.encode(text) + [tk.eot]
        if len(ids) > context_length:
            if not truncate:
                raise RuntimeError(f"Input {text} is too long for context length {context_length}")
            ids = ids[:context_length]
            ids[-1] = tk.eot
        out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return out
