"""Input pipeline for the hot path: arrow reader + CLIP transform + collate + tokenisation, producing
the batch dict of the drop-in boundary (8b) with the NEXT batch decoded, resized and uploaded while the current one
trains.

Reference pieces restated (host side, Python like the reference's):
  * `BaseDataset` (m3ae/datasets/base_dataset.py:12-228): `{data_dir}/{name}.arrow` written by prepro/make_arrow.py
    (:126-204: columns image, questions, answers, answer_labels, answer_scores, image_id, question_id, answer_type,
    split), one sample per (image row, question index) (`index_mapper`, :72-81);
  * `VQAVQARADDataset.__getitem__` (vqa_vqa_rad_dataset.py:24-43);
  * `clip_transform` (transforms/transform.py:60-67): PIL RGBA -> `Resize(size, BICUBIC)` (shorter side, torchvision's
    integer rounding) -> `CenterCrop(size)` -> RGB -> ToTensor -> Normalize(CLIP mean / std);
  * `collate` (base_dataset.py:165-228): fine-tuning keys, and with an `MLMCollator` the pre-training fields
    `text_ids_mlm` / `text_labels_mlm`;
  * the masked-language-model collators the datamodule picks (base_datamodule.py:62-69, third-party transformers==4.6.0
    `DataCollatorForWholeWordMask` / `DataCollatorForLanguageModeling`; the reference vendors the same file as
    m3ae/utils/data_collator.py:290-496) -> `MLMCollator`.

MI355X side, `image_transform="host"` (the default): decode + bicubic resize run on host cores (PIL releases the GIL; a
thread pool of `num_workers`), the crop is handed over as uint8 NHWC in PINNED memory (a quarter of the fp32 bytes over
PCIe), copied on a side HIP stream, and ToTensor + Normalize run in one kernel on the GPU (`m3ae_image_normalize_u8`,
same IEEE arithmetic as torch: bit-equal to the reference's tensor).  `ArrowDataModule.train_batches` keeps `prefetch`
batches in flight.

`image_transform="device"`: only the decode stays on the host.  The workers hand over the decoded RGB bytes of every
opaque image, `collate_host` packs a batch's sources with their resample plan and coefficient tables
(m3ae_amd/resample.py) into one pinned upload, and `m3ae_image_resample_u8` (csrc/image.hip) runs Pillow's fixed-point
bicubic resize, the centre crop and ToTensor + Normalize on the GPU: the same integer arithmetic, so the batch is
bit-identical to the host path's.  An image with real transparency (Pillow premultiplies it around the resize) or beyond
the staging caps is transformed on the host as before and joins the batch as a size x size source with identity tables;
`ArrowDataModule.transform_stats` counts both routes.

`image_dedup=True` (VQA tables; off by default): Med-VQA data asks many questions about few images, so a batch is collated per
distinct (table, image row) -- `collate_dedup`: the workers decode and transform every distinct image of the batch once,
`image_u8` is [U, ...] (the device transform receives U sources), and the batch carries `image_index` (int64 [B]: the image row
of every sample) with the index tables `M3AETransformerSS.infer` needs (`image_groups`, ops.ImageGroups; pinned, uploaded with
the batch).  The samples of a batch and their order are those of the plain path.  `transform_stats.decodes` counts the decodes.

`train_transform_keys=["clip_resizedcrop"]` (named config `clip_resizedcrop`; transforms/transform.py:70-77): every image a TRAIN
split loads under `train_batches(epoch)` is cropped to a box of `resample.random_resized_crop_box` and the box resized to size x
size (`clip_resized_crop`), under either `image_transform`; the device transform gets the whole source plus the box and builds the
box's coefficient tables on the GPU (`m3ae_image_resample_tables`).  The box is drawn from a `random.Random` keyed by (seed, epoch,
global sample index, slot) -- slot 0 the sample's image, 1 + i its i-th false image; the reference, too, draws per loaded image --
or, under `image_dedup`, by (seed, epoch, image key): one box per distinct image and epoch (the datasets' `box_key`).  No global
generator is read, so epoch e gives the same batches whenever it runs.  `val_batches` and the val / test sets never crop.

`randaug=True` (off by default; with the `clip` tail the reference's `clip_randaug`, transforms/transform.py:80-91): every image a
TRAIN split loads under `train_batches(epoch)` is converted to RGB and run through `RandAugment(2, 9)` (m3ae_amd/randaug.py) in
front of whichever tail `train_transform_keys` names.  The two operations and their signs are drawn by the crop box's rule from a
generator of their own (randaug.aug_rng on the same key), so the box of `clip_resizedcrop` is the one it would be without them.
"host": Pillow runs the operations on the loader threads.  "device": the pack carries an augment plan and csrc/randaug.hip runs the
operations on the uploaded source bytes in front of the resample -- the same bytes, so the batches are equal.  An image beyond the
staging caps is augmented and transformed on the host and joins with an identity record.
"""
import ctypes as C
import io
import os
import queue
import random
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, randaug, resample
from .synth import CLIP_MEAN, CLIP_STD


# ------------------------------------------------------------------------------------------------------------
# transform (host part)
# ------------------------------------------------------------------------------------------------------------
def clip_resize_crop(img, size):
    """PIL image -> uint8 [size, size, 3]: transform.py:60-64 (Resize BICUBIC on the RGBA image, CenterCrop, RGB)."""
    from PIL import Image
    img = img.convert("RGBA")                      # base_dataset.py:92-93
    w, h = img.size
    if w <= h:                                     # torchvision Resize(int): shorter side -> size, long side truncated
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    if (nw, nh) != (w, h):
        img = img.resize((nw, nh), Image.BICUBIC)
    top, left = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))
    img = img.crop((left, top, left + size, top + size)).convert("RGB")
    return np.array(img, dtype=np.uint8)  # a writable copy (torch.from_numpy)


def clip_resized_crop(img, size, box):
    """PIL image, box (left, top, cw, ch) -> uint8 [size, size, 3]: transform.py:70-74 with the box given -- torchvision's
    `resized_crop` (crop, then resize to size x size, BICUBIC) on the RGBA image; CenterCrop(size) is then the identity; RGB."""
    from PIL import Image
    left, top, cw, ch = box
    img = img.convert("RGBA").crop((left, top, left + cw, top + ch)).resize((size, size), Image.BICUBIC).convert("RGB")
    return np.array(img, dtype=np.uint8)


class TransformStats(dict):
    """{"device": n, "fallback": n}: images the device transform took from their source bytes / images the host transformed
    (real transparency, or beyond the staging caps); counted from the loader's worker threads."""

    def __init__(self):
        super().__init__(device=0, fallback=0)
        self._lock = threading.Lock()
        self.decodes = 0   # images decoded, either transform (an attribute: the dict holds the device transform's routes alone)

    def count(self, route):
        with self._lock:
            self[route] += 1

    def count_decode(self):
        with self._lock:
            self.decodes += 1


def load_image_u8(raw, size, image_transform="host", stats=None, box_key=None, aug_key=None):
    """Encoded image bytes -> uint8 [size, size, 3] (the finished crop, "host") or the source the device transform resizes
    ("device": uint8 [h, w, 3], or the host-made crop of an image it does not take).
    `box_key` (a train split under "clip_resizedcrop"; a tuple of ints / strings): the image is cropped to the box that key draws
    (resample.box_rng, random_resized_crop_box) and the box resized; the device route then returns (source, box) for
    `resample.pack_batch(..., boxes=)`.
    `aug_key` (a train split under `randaug`): the image is converted to RGB and run through the two operations that key draws
    (randaug.aug_rng, randaug.draw) first; the device route then returns (source, box or None, operations or None) for
    `resample.pack_batch(..., augs=)`."""
    from PIL import Image
    img = Image.open(io.BytesIO(raw))
    if stats is not None:
        stats.count_decode()
    box = None if box_key is None else resample.random_resized_crop_box(*img.size, resample.box_rng(*box_key))
    ops = None if aug_key is None else randaug.draw(randaug.aug_rng(*aug_key))
    if image_transform != "device":
        if ops is not None:
            img = randaug.augment_pil(img, ops)
        return clip_resize_crop(img, size) if box is None else clip_resized_crop(img, size, box)
    route, *a = resample.prepare(img, size, box, ops)
    if stats is not None:
        stats.count(route)
    if ops is not None:
        return tuple(a)
    return a[0] if box is None else tuple(a)


def normalize_on_device(u8_nhwc, stream=None):
    """uint8 [B, H, W, 3] (device) -> fp32 [B, 3, H, W]: ToTensor + Normalize in one kernel."""
    B, H, W, _ = u8_nhwc.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=u8_nhwc.device)
    mean = (C.c_float * 3)(*CLIP_MEAN)
    std = (C.c_float * 3)(*CLIP_STD)
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    _lib.check(_lib.lib().m3ae_image_normalize_u8(C.c_void_p(u8_nhwc.data_ptr()), C.c_void_p(out.data_ptr()), B, H, W,
                                                  mean, std, s), "m3ae_image_normalize_u8")
    return out


# ------------------------------------------------------------------------------------------------------------
# tokenizer
# ------------------------------------------------------------------------------------------------------------
def load_tokenizer(cfg):
    """base_datamodule.py:13-26: `RobertaTokenizerFast.from_pretrained(path, local_files_only=True)`."""
    name = cfg["tokenizer"]
    from transformers import BertTokenizerFast, RobertaTokenizerFast
    if "roberta" in name:
        return RobertaTokenizerFast.from_pretrained(name, local_files_only=True)
    return BertTokenizerFast.from_pretrained(name, do_lower_case="uncased" in name, local_files_only=True)


# ------------------------------------------------------------------------------------------------------------
# masked-language-model collation (pre-training batches)
# ------------------------------------------------------------------------------------------------------------
class MLMCollator:
    """`mlm_collator` of base_datamodule.py:62-69, restated (host side; consumes Python's `random` and torch's CPU
    generator in the release's order, so a seeded run reproduces the release's draws -- tests/golden/mlm_collate.npz).

    whole_word=True (config.py:40): data_collator.py:381-496.  Per example, candidate words are runs of a token followed
    by its "##" continuations; "[CLS]" / "[SEP]" are skipped BY NAME, so with the RoBERTa vocabulary (no "##", specials
    called <s> </s> <pad>) every position -- specials and padding included -- is a one-token candidate.  The candidates are
    shuffled and taken until max(1, round(len * p)) positions are covered (len = the PADDED length the dataset
    produced, base_dataset.py:154-163), then specials and padding are struck from the selection: a short question
    ends up with fewer masked tokens than the count suggests.  Quirks kept as they are.
    whole_word=False: data_collator.py:290-378, Bernoulli(p) per non-special position.
    Both: selected positions keep their id as label (-100 elsewhere) and are rewritten 80 % -> <mask>, 10 % -> a uniform
    random id, 10 % unchanged."""

    def __init__(self, tokenizer, mlm_probability=0.15, whole_word=True, max_predictions=512):
        self.tok, self.p, self.whole_word, self.max_predictions = tokenizer, mlm_probability, whole_word, max_predictions
        if getattr(tokenizer, "mask_token_id", None) is None:
            raise ValueError("masked language modelling needs a tokenizer with a mask token")

    def _pad(self, rows):
        """_collate_batch (data_collator.py:253-287): right-pad with pad_token_id to the longest row."""
        n = max(len(r) for r in rows)
        out = torch.full((len(rows), n), int(self.tok.pad_token_id), dtype=torch.long)
        for i, r in enumerate(rows):
            out[i, : len(r)] = torch.as_tensor(r, dtype=torch.long)
        return out

    def _special(self, ids):
        return torch.tensor([self.tok.get_special_tokens_mask(r, already_has_special_tokens=True) for r in ids.tolist()],
                            dtype=torch.bool)

    def _word_selection(self, tokens):
        words = []
        for i, t in enumerate(tokens):
            if t in ("[CLS]", "[SEP]"):
                continue
            if words and t.startswith("##"):
                words[-1].append(i)
            else:
                words.append([i])
        random.shuffle(words)
        budget = min(self.max_predictions, max(1, int(round(len(tokens) * self.p))))
        chosen = []
        for w in words:
            if len(chosen) >= budget:
                break
            if len(chosen) + len(w) > budget or any(i in chosen for i in w):
                continue
            chosen.extend(w)
        sel = [0] * len(tokens)
        for i in chosen:
            sel[i] = 1
        return sel

    def __call__(self, encodings):
        rows = [list(e["input_ids"]) if isinstance(e, dict) else list(e) for e in encodings]
        ids = self._pad(rows)
        labels = ids.clone()
        if self.whole_word:
            # the selection rows are padded with pad_token_id too (any non-zero reads as "selected"); padding is struck below
            picked = self._pad([self._word_selection(self.tok.convert_ids_to_tokens(r)) for r in rows])
            picked.masked_fill_(self._special(labels), 0)
            picked.masked_fill_(labels.eq(int(self.tok.pad_token_id)), 0)
            picked = picked.bool()
        else:
            prob = torch.full(labels.shape, self.p)
            prob.masked_fill_(self._special(labels), 0.0)
            picked = torch.bernoulli(prob).bool()
        labels[~picked] = -100
        to_mask = torch.bernoulli(torch.full(labels.shape, 0.8)).bool() & picked
        ids[to_mask] = int(self.tok.mask_token_id)
        to_random = torch.bernoulli(torch.full(labels.shape, 0.5)).bool() & picked & ~to_mask
        ids[to_random] = torch.randint(len(self.tok), labels.shape, dtype=torch.long)[to_random]
        return {"input_ids": ids, "labels": labels}


# ------------------------------------------------------------------------------------------------------------
# dataset
# ------------------------------------------------------------------------------------------------------------
def _keyed_load(ds, row, key):
    """`ds.image_u8(row)` under the key of one loaded image: it draws the crop box of a dataset that crops and, through a generator
    of their own, the RandAugment operations of a dataset with `randaug`."""
    kw = {"aug_key": key} if ds.randaug else {}
    return ds.image_u8(row, key if ds.crop else None, **kw)


class ArrowVQADataset:
    """BaseDataset + VQAVQARADDataset for `{data_dir}/vqa_vqa_rad_{split}.arrow` (or any `names`)."""

    def __init__(self, data_dir, split, image_size, max_text_len, tokenizer, names=None, image_transform="host", stats=None,
                 train_transform="clip", seed=0, box_key="sample", randaug=False):
        import pyarrow as pa
        self.image_transform, self.stats = image_transform, stats
        # the random resized crop and RandAugment: train split only (base_dataset.py:39-41), and only for a fetch that names its epoch
        self.crop, self.randaug = split == "train" and train_transform == "clip_resizedcrop", split == "train" and bool(randaug)
        self.augment, self.seed, self.box_key = self.crop or self.randaug, seed, box_key
        self.names = names or [f"vqa_vqa_rad_{split}"]
        tables = []
        for name in self.names:
            path = os.path.join(data_dir, f"{name}.arrow")
            if os.path.isfile(path):
                tables.append(pa.ipc.RecordBatchFileReader(pa.memory_map(path, "r")).read_all())
        if not tables:
            raise FileNotFoundError(f"no arrow table for {self.names} under {data_dir!r}")
        self.table = pa.concat_tables(tables)
        self.image_size, self.max_text_len, self.tokenizer = image_size, max_text_len, tokenizer
        self.all_texts = self.table["questions"].to_pylist()
        self.index_mapper = [(i, j) for i, texts in enumerate(self.all_texts) for j in range(len(texts))]

    def __len__(self):
        return len(self.index_mapper)

    def image_u8(self, row, box_key=None, aug_key=None):
        return load_image_u8(self.table["image"][row].as_py(), self.image_size, self.image_transform, self.stats, box_key, aug_key)

    def get(self, index, epoch=None, key_index=None):
        """Sample `index`; with `epoch` (train_batches) on an augmenting dataset its image is cropped to the box of (seed, epoch,
        key_index or index, slot 0) -- or of its image key, `box_key == "image"`."""
        sample, key = self.sample_without_image(index)
        if not self.augment or epoch is None:
            return {"image_u8": self.image_u8(key[1]), **sample}
        if self.box_key == "image":
            return {"image_u8": self.image_by_key(key, epoch), **sample}
        return {"image_u8": _keyed_load(self, key[1], (self.seed, epoch, index if key_index is None else key_index, 0)), **sample}

    def __getitem__(self, index):
        return self.get(index)

    def sample_without_image(self, index):
        """(the sample of `__getitem__` without its "image_u8", its image key): samples with equal keys show the same image, which
        `image_by_key` loads (collate_dedup: one decode per distinct key of a batch)."""
        row, qi = self.index_mapper[index]
        text = self.all_texts[row][qi]
        enc = self.tokenizer(text, padding="max_length", truncation=True, max_length=self.max_text_len)
        t = self.table
        return {
            "text": text,
            "input_ids": list(enc["input_ids"]),
            "attention_mask": list(enc["attention_mask"]),
            "vqa_answer": t["answers"][row][qi].as_py(),
            "vqa_labels": t["answer_labels"][row][qi].as_py(),
            "vqa_scores": t["answer_scores"][row][qi].as_py(),
            "answer_types": t["answer_type"][row][qi].as_py(),
            "qid": t["question_id"][row][qi].as_py(),
        }, ("+".join(self.names), row)

    def image_by_key(self, key, epoch=None):
        """The image of an image key; with `epoch` on an augmenting dataset, cropped to that image's box of the epoch."""
        if not self.augment or epoch is None:
            return self.image_u8(key[1])
        return _keyed_load(self, key[1], (self.seed, epoch, key))


class ArrowCaptionDataset:
    """BaseDataset + ROCODataset / MedicatDataset (pretraining_roco_dataset.py:1-21, pretraining_medicat_dataset.py:1-21):
    `{data_dir}/{name}_{split}.arrow` written by prepro/make_arrow.py:40-63 (columns image, caption [list of str], image_id,
    split), one sample per (image row, caption index) (base_dataset.py:72-81), and `get_suite` (:141-163): the image, its
    caption, and `draw_false_image` negatives drawn as `random.randint(0, len - 1)` over THIS table's samples
    (`get_false_image`, :107-111) -- Python's `random` stream, as the reference consumes it, so a seeded run reproduces the
    reference's draws.  A sample that fails to decode is replaced by a random one (:158-160)."""

    def __init__(self, data_dir, name, split, image_size, max_text_len, tokenizer, draw_false_image=0, image_transform="host",
                 stats=None, train_transform="clip", seed=0, box_key="sample", randaug=False):
        import pyarrow as pa
        self.image_transform, self.stats = image_transform, stats
        self.crop, self.randaug = split == "train" and train_transform == "clip_resizedcrop", split == "train" and bool(randaug)
        self.augment, self.seed, self.box_key = self.crop or self.randaug, seed, box_key
        assert split in ("train", "val", "test")
        self.names = [f"{name}_{split}"]
        path = os.path.join(data_dir, f"{self.names[0]}.arrow")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"no arrow table {path!r}")
        self.table = pa.ipc.RecordBatchFileReader(pa.memory_map(path, "r")).read_all()
        self.image_size, self.max_text_len, self.tokenizer = image_size, max_text_len, tokenizer
        self.draw_false_image = draw_false_image
        self.all_texts = self.table["caption"].to_pylist()
        assert isinstance(self.all_texts[0][0], str)
        self.index_mapper = [(i, j) for i, texts in enumerate(self.all_texts) for j in range(len(texts))]

    def __len__(self):
        return len(self.index_mapper)

    def image_u8(self, row, box_key=None, aug_key=None):
        return load_image_u8(self.table["image"][row].as_py(), self.image_size, self.image_transform, self.stats, box_key, aug_key)

    def get_suite(self, index, epoch=None, key_index=None):
        """`epoch` (train_batches) on an augmenting dataset: every image loaded is cropped to a box of its own -- (seed, epoch,
        key_index or index, slot), slot 0 the sample's image and 1 + i its i-th false image; per image key, `box_key == "image"`."""
        if not self.augment or epoch is None:
            load = lambda row, slot: self.image_u8(row)
        elif self.box_key == "image":
            load = lambda row, slot: _keyed_load(self, row, (self.seed, epoch, (self.names[0], row)))
        else:
            key = index if key_index is None else key_index
            load = lambda row, slot: _keyed_load(self, row, (self.seed, epoch, key, slot))
        while True:
            try:
                row, ci = self.index_mapper[index]
                text = self.all_texts[row][ci]
                enc = self.tokenizer(text, padding="max_length", truncation=True, max_length=self.max_text_len)
                ret = {"image_u8": load(row, 0), "text": text, "input_ids": list(enc["input_ids"]),
                       "attention_mask": list(enc["attention_mask"]), "img_index": row, "cap_index": ci,
                       "raw_index": index, "replica": ci > 0}
                for rep in range(self.draw_false_image):
                    frow, _ = self.index_mapper[random.randint(0, len(self.index_mapper) - 1)]
                    ret[f"false_image_u8_{rep}"] = load(frow, 1 + rep)
                return ret
            except Exception as e:  # noqa: BLE001  (base_dataset.py:158-160)
                print(f"Error while read file idx {index} in {self.names[0]} -> {e}")
                index = random.randint(0, len(self.index_mapper) - 1)

    get = get_suite

    def __getitem__(self, index):
        return self.get_suite(index)


class ConcatDataset:
    """torch.utils.data.ConcatDataset as MTDataModule uses it (multitask_datamodule.py:36-40): datasets back to back."""

    def __init__(self, parts):
        self.parts = list(parts)
        self.augment = any(getattr(p, "augment", False) for p in self.parts)
        self.ends = np.cumsum([len(p) for p in self.parts]).tolist()

    def __len__(self):
        return self.ends[-1] if self.ends else 0

    def get(self, index, epoch=None):
        """Sample `index`; `epoch` reaches the part with the GLOBAL index as the key of its crop boxes."""
        for p, end in zip(self.parts, self.ends):
            if index < end:
                return p.get(index - (end - len(p)), epoch, key_index=index)
        raise IndexError(index)

    def __getitem__(self, index):
        return self.get(index)


def collate_host(samples, pin=True, mlm_collator=None, resample_size=None, pmap=map, images=None, image_index=None):
    """base_dataset.py:165-228: images stacked as uint8 NHWC, ids / masks as int64 tensors; with `mlm_collator` also
    `text_ids_mlm` / `text_labels_mlm` (:202-209; the reference always computes them, the fine-tuning step never reads
    them).  `resample_size` (image_transform="device"): the samples carry sources of any sizes; each image key becomes a
    pack (resample.pack_batch: source bytes, plan, tables) for the device transform to that size, its copies run through `pmap`.
    `images` + `image_index` (collate_dedup): the samples carry no image; `image_u8` is built from the U distinct `images` and the
    batch gets `image_index` (sample -> image row) and `image_groups` (ops.image_groups: the tables infer() reads)."""
    B = len(samples)
    S = max(len(s["input_ids"]) for s in samples)
    if resample_size:
        def stack_list(arrays):   # (source, box) pairs under "clip_resizedcrop", (source, box or None, operations) under randaug
            if not isinstance(arrays[0], tuple):
                return resample.pack_batch(arrays, resample_size, pin=pin, pmap=pmap)
            boxes = None if arrays[0][1] is None else [a[1] for a in arrays]
            augs = [a[2] for a in arrays] if len(arrays[0]) > 2 else None
            return resample.pack_batch([a[0] for a in arrays], resample_size, pin=pin, pmap=pmap, boxes=boxes, augs=augs)
    else:
        stack_list = lambda arrays: torch.from_numpy(np.stack(arrays))
    stack = lambda k: stack_list([s[k] for s in samples])
    img = stack("image_u8") if images is None else stack_list(list(images))
    ids = torch.zeros((B, S), dtype=torch.long)
    mask = torch.zeros((B, S), dtype=torch.long)
    for i, s in enumerate(samples):
        ids[i, : len(s["input_ids"])] = torch.tensor(s["input_ids"])
        mask[i, : len(s["attention_mask"])] = torch.tensor(s["attention_mask"])
    extra = {}
    if mlm_collator is not None:
        m = mlm_collator([{"input_ids": s["input_ids"]} for s in samples])
        extra = {"text_ids_mlm": m["input_ids"], "text_labels_mlm": m["labels"]}
    for k in sorted(samples[0]):   # the negatives of the image-text matching objective (base_dataset.py:107-111, :173-195)
        if k.startswith("false_image_u8_"):
            extra[k] = stack(k)
    if pin and torch.cuda.is_available():
        _pin = lambda v: v.pin_memory() if isinstance(v, torch.Tensor) else v   # a pack is pinned as it is built
        img, ids, mask = _pin(img), ids.pin_memory(), mask.pin_memory()
        extra = {k: _pin(v) for k, v in extra.items()}
    out = {"image_u8": img, "text_ids": ids, "text_masks": mask, **extra, "text": [s["text"] for s in samples]}
    if images is not None:
        from . import ops
        groups = ops.image_groups(np.asarray(image_index, dtype=np.int64), n_images=len(images), pin=pin)
        out["image_index"], out["image_groups"] = groups.index, groups
    for k in ("vqa_answer", "vqa_labels", "vqa_scores", "answer_types", "qid", "img_index", "cap_index", "raw_index",
              "replica"):
        if k in samples[0]:
            out[k] = [s[k] for s in samples]
    return out


def collate_dedup(ds, indices, pmap=map, epoch=None, **collate_kw):
    """`collate_host` of the samples `indices` of a dataset with `sample_without_image` / `image_by_key` (ArrowVQADataset), per
    distinct image: every distinct (table, image row) of the batch is loaded ONCE (through `pmap`: the loader's thread pool), in
    the order of its first sample.  Same samples, same order, same keys as the plain collate plus `image_index` / `image_groups`;
    `image_u8[image_index]` is the plain batch's `image_u8`.  `epoch` (train_batches): an augmenting dataset crops every distinct
    image to its box of that epoch -- the plain batch of a dataset with `box_key == "image"`."""
    metas = list(pmap(ds.sample_without_image, indices))
    rows, index = {}, []
    for _, key in metas:
        index.append(rows.setdefault(key, len(rows)))
    images = list(pmap(ds.image_by_key if epoch is None else (lambda key: ds.image_by_key(key, epoch)), list(rows)))
    return collate_host([m[0] for m in metas], pmap=pmap, images=images, image_index=index, **collate_kw)


def to_device_batch(hb, device, copy_stream=None):
    """Upload a host batch (pinned) and finish the transform on the GPU -> the 8b batch dict."""
    cur = torch.cuda.current_stream()
    cs = copy_stream or cur
    _up = lambda v: v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else resample.upload(v, device)
    with torch.cuda.stream(cs):
        u8 = _up(hb["image_u8"])
        ids = hb["text_ids"].to(device, non_blocking=True)
        mask = hb["text_masks"].to(device, non_blocking=True)
        ev = torch.cuda.Event()
        mlm = {k: hb[k].to(device, non_blocking=True) for k in ("text_ids_mlm", "text_labels_mlm") if k in hb}
        fal = {"_" + k: _up(hb[k]) for k in hb if k.startswith("false_image_u8_")}
        grp = {}
        if "image_groups" in hb:   # de-duplicated batch: the pinned index tables ride with the upload
            g = hb["image_groups"].to(device)
            grp = {"image_index": g.index, "image_groups": g}
        ev.record(cs)
    out = {k: v for k, v in hb.items() if k not in ("image_u8", "text_ids", "text_masks", "text_ids_mlm", "text_labels_mlm",
                                                     "image_index", "image_groups")
           and not k.startswith("false_image_u8_")}
    out.update(_u8=u8, text_ids=ids, text_masks=mask, text_labels=None, _ready=ev, **mlm, **fal, **grp)
    return out


def _finish_image(u8, cur):
    """The uploaded crop -- or, under image_transform="device", the uploaded pack -- to the fp32 image, on the compute stream."""
    if isinstance(u8, torch.Tensor):
        u8.record_stream(cur)
        return normalize_on_device(u8)
    for k in ("src", "plan", "tab", "aug"):   # uploaded on the copy stream, read here (a pack with boxes has no uploaded tables)
        if k in u8:
            u8[k].record_stream(cur)
    return resample.resample_on_device(u8)


def finish_batch(db):
    """Called on the compute stream right before the step: wait for the upload, resize (device transform) / normalise,
    build labels."""
    cur = torch.cuda.current_stream()
    cur.wait_event(db.pop("_ready"))
    db["image"] = [_finish_image(db.pop("_u8"), cur)]
    for k in [k for k in db if k.startswith("_false_image_u8_")]:
        db["false_image_" + k[len("_false_image_u8_"):]] = [_finish_image(db.pop(k), cur)]
    db["text_labels"] = torch.full_like(db["text_ids"], -100)
    for t in db.values():   # every tensor uploaded on the copy stream (text_ids_mlm / text_labels_mlm included) is now used here
        if isinstance(t, torch.Tensor) and t.is_cuda:
            t.record_stream(cur)
    if "image_groups" in db:
        for t in db["image_groups"].tensors():
            t.record_stream(cur)
    return db


# ------------------------------------------------------------------------------------------------------------
# datamodule
# ------------------------------------------------------------------------------------------------------------
class ArrowDataModule:
    """MTDataModule / BaseDataModule for the hot path: DistributedSampler-style sharding (seeded shuffle per epoch,
    multitask_datamodule.py:44-48), `per_gpu_batchsize` batches, background decode + upload."""

    def __init__(self, cfg, rank=0, world=1, device="cuda", tokenizer=None, prefetch=3, head="cls"):
        self.cfg, self.rank, self.world, self.device, self.head = cfg, rank, world, device, head
        self.B = cfg["per_gpu_batchsize"]
        self.tokenizer = tokenizer or load_tokenizer(cfg)
        root = cfg["data_root"]
        names = list(cfg.get("datasets") or ["vqa_vqa_rad"])
        self.image_transform = cfg.get("image_transform", "host")
        if self.image_transform not in ("host", "device"):
            raise ValueError(f"image_transform must be 'host' or 'device', not {self.image_transform!r}")
        self.transform_stats = TransformStats()
        self.image_dedup = bool(cfg.get("image_dedup", False))
        loss_names = cfg.get("loss_names", {})
        if self.image_dedup and any(loss_names.get(k, 0) > 0 for k in ("mim", "itm")):
            raise ValueError("image_dedup=True cannot be combined with the mim / itm objectives (loss_names): they read the image "
                             "pixels per sample")
        from .config import randaug_enabled, transform_keys
        self.train_transform = transform_keys(cfg)[0]
        # one crop box (and one RandAugment draw) per distinct image and epoch under image_dedup, else one per loaded image (the
        # reference's rule)
        tf = dict(image_transform=self.image_transform, stats=self.transform_stats, train_transform=self.train_transform,
                  seed=cfg["seed"], box_key="image" if self.image_dedup else "sample", randaug=randaug_enabled(cfg))
        if any(n in ("roco", "medicat") for n in names):   # the pre-training caption tables (config.py:22,31: draw_false_image = 1)
            mk = lambda split: ConcatDataset([ArrowCaptionDataset(root, n, split, cfg["image_size"], cfg["max_text_len"],
                                                                  self.tokenizer, cfg.get("draw_false_image", 0), **tf)
                                              for n in names])
        else:
            mk = lambda split: ArrowVQADataset(root, split, cfg["image_size"], cfg["max_text_len"], self.tokenizer, **tf)
        self.train_set = mk("train")
        self.val_set = self._try(mk, "val") or self.train_set
        self.test_set = self._try(mk, "test") or self.val_set
        self.train_samples, self.val_samples = len(self.train_set), len(self.val_set)
        self.workers = max(int(cfg.get("num_workers", 8)), 1)
        self.prefetch = prefetch
        self.copy_stream = torch.cuda.Stream(device=device) if torch.cuda.is_available() else None
        # base_datamodule.py:62-69; the reference builds it for every task, only the MLM objective reads its output
        self.mlm_collator = None
        if cfg.get("loss_names", {}).get("mlm", 0) > 0:
            self.mlm_collator = MLMCollator(self.tokenizer, cfg.get("mlm_prob", 0.15), cfg.get("whole_word_masking", True))

    @staticmethod
    def _try(mk, split):
        try:
            return mk(split)
        except FileNotFoundError:
            return None

    def _indices(self, ds, epoch, shuffle):
        idx = list(range(len(ds)))
        if shuffle:
            random.Random(self.cfg["seed"] * 1000 + epoch).shuffle(idx)
        total = (len(idx) + self.world - 1) // self.world * self.world  # DistributedSampler pads by wrapping around
        idx += idx[: total - len(idx)]
        return idx[self.rank::self.world]

    def _stream(self, ds, idx, drop_last, epoch=None):
        """Generator of device batches; host decode runs `prefetch` batches ahead in a thread pool.  `epoch`: the training epoch
        the samples are fetched for (the key of the random resized crop's boxes); None never crops."""
        chunks = [idx[i:i + self.B] for i in range(0, len(idx), self.B)]
        if drop_last:
            chunks = [c for c in chunks if len(c) == self.B]
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        dedup = self.image_dedup and hasattr(ds, "sample_without_image")   # (the caption tables ignore the flag)
        if not getattr(ds, "augment", False):
            epoch = None
        fetch = ds.__getitem__ if epoch is None else (lambda i: ds.get(i, epoch))

        def producer():
            kw = dict(mlm_collator=self.mlm_collator,
                      resample_size=self.cfg["image_size"] if self.image_transform == "device" else None)
            with ThreadPoolExecutor(self.workers) as pool:
                for c in chunks:
                    if stop.is_set():
                        break
                    if dedup:
                        q.put(collate_dedup(ds, c, pmap=pool.map, epoch=epoch, **kw))
                    else:
                        q.put(collate_host(list(pool.map(fetch, c)), pmap=pool.map, **kw))
            q.put(None)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        pending = None
        try:
            while True:
                hb = q.get()
                nxt = None if hb is None else to_device_batch(hb, self.device, self.copy_stream)
                if pending is not None:
                    yield finish_batch(pending)   # its upload was issued one batch ago
                if nxt is None:
                    break
                pending = nxt
        finally:
            stop.set()
            while th.is_alive():
                try:
                    q.get_nowait()
                except queue.Empty:
                    th.join(timeout=0.05)

    def train_batches(self, epoch):
        return self._stream(self.train_set, self._indices(self.train_set, epoch, True), drop_last=False, epoch=epoch)

    def val_batches(self):
        return self._stream(self.val_set, self._indices(self.val_set, 0, False), drop_last=False)
