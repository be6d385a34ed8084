"""Trainer / entry-point shim: what `main.py` / `main_t5_m3ae.py` + `pl.Trainer` do for the hot path,
without Lightning or sacred.

    python main.py with data_root=synthetic num_gpus=1 num_nodes=1 task_finetune_vqa_vqa_rad \
        per_gpu_batchsize=64 clip16 text_roberta image_size=384 tokenizer=downloaded/roberta-base

accepts the argument grammar of run_scripts/*.sh (`config.parse_cli`), and reproduces the reference's training
arithmetic around `training_step`:

* gradient accumulation `grad_steps = max(batch_size // (per_gpu_batchsize * num_gpus * num_nodes), 1)` (main.py:50,70):
  the loss of every micro-batch is divided by `grad_steps` (Lightning's `accumulate_grad_batches`), gradients add up
  in place in the flat buffer, the gradient all-reduce runs on the LAST micro-batch only (ddp.FlatGradReducer);
* `max_steps` optimizer steps, or `max_epoch` epochs when `max_steps` is None / -1 (main.py:51-52);
* the 6-group optimizer of `optim_type` -- AdamW, Adam or SGD with momentum (m3ae_utils.py:203-210) -- + polynomial schedule
  stepped once per optimizer step (m3ae_utils.py:112-242, ParamStore.optimizer_step through the Flat* optimizer);
* `gradient_clip_val` (Lightning's Trainer flag; 0 = off): clipping by global norm and the non-finite step guard happen inside
  `optimizer.step()`, after the gradient all-reduce, once per accumulation window (ParamStore.update_apply); the periodic log line
  then also shows the gradient norm, the factor applied and the number of skipped steps;
* `ema_decay` (not in the reference; 0 = off): an exponential moving average of the trainable weights, updated inside
  `optimizer.step()` (ParamStore.update_range).  With `ema_eval` validation and test run on the averaged weights
  (ParamStore.ema_weights), so `best.ckpt` is chosen by their metric and the log line says `(ema)`; checkpoints keep `state_dict` as
  the raw weights -- `resume` stays exact -- and carry `ema_state_dict` / `ema_updates` next to it (`load_ema` reads them);
* `lora_rank` (not in the reference; 0 = off): LoRA in merged form (m3ae_amd/lora.py).  `optimizer.step()` projects the adapter
  gradients out of the weight gradients, steps adapters and heads and merges; checkpoints keep `state_dict` as the merged weights
  and carry `lora_state_dict` (+ the adapters' moments unless weights-only); next to each checkpoint an adapter-only `*.lora.pt`
  is written, which `lora_path` loads onto the base from `load_path`;
* validation every `val_check_interval` of an epoch with the VQA score `val/the_metric` (my_metrics.py:58-83), best +
  last checkpoints (`ModelCheckpoint(save_top_k=1, monitor="val/the_metric", mode="max", save_last=True)`,
  main.py:36-43) written as `{"state_dict": ...}` with the REFERENCE's key names, so the files load in the upstream
  code and upstream checkpoints load here (`load_path`); `save_weights_only` when "finetune" is in `exp_name`; with
  `vqa_metrics=device` the score is kept on the GPU (m3ae_amd/metrics.py) and validation also reports the closed / open scores
  and the score within the top `eval_topk` answers, `test()` token exact match for the generator heads; with
  `pretrain_metrics=device` a validation pass of the pre-training objectives also reports MLM / ITM accuracy, MLM accuracy within
  the top `eval_topk` tokens, perplexity and the mean loss per objective (the reference's `Accuracy` / `Scalar` logs,
  objectives.py:32-36, :70-74, :114-117), accumulated on the GPU; the monitored quantity stays the negative summed loss;
* one process per GPU: launched under `python -m torch.distributed.run --nproc-per-node N main.py with ...`
  (RANK / LOCAL_RANK / WORLD_SIZE), RCCL through `torch.distributed`; `num_gpus` * `num_nodes` must equal the world.

Data: `data_root=<dir with vqa_vqa_rad_{train,val,test}.arrow>` runs the arrow input pipeline (m3ae_amd/data.py, SURVEY
8f-2: host decode + bicubic resize in a thread pool, pinned uint8 upload on a side stream, ToTensor + Normalize on
the GPU; with `image_transform=device` the resize and the crop run on the GPU too, from the decoded bytes, and give
bit-identical batches; with `image_dedup=True` a batch carries each distinct image once and the image tower runs once per distinct
image); `data_root=synthetic` (or empty) selects `SyntheticDataModule`, which serves deterministic batches with the
same collate schema (base_dataset.py:165-228).
"""
import json
import math
import os
import sys
import time

import torch
import torch.distributed as dist

from . import config as config_mod
from . import metrics as metrics_mod
from . import ops, synth
from .ddp import FlatGradReducer
from .modules.objectives import build_vqa_targets


def log(msg, rank=0):
    if rank == 0:
        print(f"[m3ae] {msg}", file=sys.stderr, flush=True)


def grad_steps_of(cfg, world):
    """main.py:50 (num_gpus * num_nodes is the world size under Lightning ddp)."""
    return max(cfg["batch_size"] // (cfg["per_gpu_batchsize"] * world), 1)


def plan(cfg, world, train_samples):
    """Optimizer-step budget exactly as main.py:49-52 + Lightning derive it."""
    gs = grad_steps_of(cfg, world)
    # len(train_dataloader): DistributedSampler gives every rank ceil(n / world) samples, the loader keeps the ragged last
    # batch (drop_last=False) -> ceil; Lightning steps the optimizer on an epoch's last batch even when the accumulation
    # window is incomplete -> ceil again for the steps of an epoch
    micro_per_epoch = max(math.ceil(math.ceil(train_samples / world) / cfg["per_gpu_batchsize"]), 1)
    steps_per_epoch = max(math.ceil(micro_per_epoch / gs), 1)
    ms = cfg["max_steps"]
    if ms is None or ms < 0:
        # m3ae_utils.py:212-217: len(train_dataloader) * max_epochs // accumulate_grad_batches
        max_steps, max_epochs = max(micro_per_epoch * cfg["max_epoch"] // gs, 1), cfg["max_epoch"]
    else:
        max_steps, max_epochs = ms, 1000
    return dict(grad_steps=gs, micro_per_epoch=micro_per_epoch, steps_per_epoch=steps_per_epoch, max_steps=max_steps,
                max_epochs=max_epochs)


class SyntheticDataModule:
    """Stand-in for MTDataModule (multitask_datamodule.py:11-82): a fixed pool of deterministic batches with the
    reference collate schema, sharded by rank.  `train_samples` mimics the dataset length (VQA-RAD train: 3064)."""

    def __init__(self, cfg, rank=0, world=1, device="cuda", head="cls", pool=4, train_samples=None, val_samples=None):
        self.cfg, self.rank, self.world, self.device, self.head = cfg, rank, world, device, head
        self.B = cfg["per_gpu_batchsize"]
        self.train_samples = train_samples or cfg.get("synthetic_train_samples", 3064)
        self.val_samples = val_samples or cfg.get("synthetic_val_samples", 451)
        self.pretrain = any(cfg["loss_names"][k] > 0 for k in ("mlm", "mim", "itm"))
        self.pool = [self._make(i) for i in range(pool)]
        self.val_pool = [self._make(1000 + i) for i in range(2)]

    def _make(self, idx):
        c = self.cfg
        b = synth.synthetic_batch(self.B, text_len=c["max_text_len"], image_size=c["image_size"],
                                  vocab_size=c["vocab_size"], label_size=c["vqa_label_size"],
                                  rank=self.rank + self.world * idx, device=self.device, pretrain=self.pretrain)
        if self.head == "t5":
            lab = synth.det_randint("t5_labels", 2, 32128, (self.B, 6), salt=31 + self.rank + self.world * idx)
            lab[:, -1] = 1
            b["t5_labels"] = lab.to(self.device)
        if self.head == "decoder":  # [CLS] answer tokens [SEP] [PAD]... with BERT's special ids (m3ae_decoder.py:336-342)
            import torch
            T = 6
            ids = synth.det_randint("dec_tokens", 1000, 30522, (self.B, T), salt=37 + self.rank + self.world * idx)
            n = synth.det_randint("dec_len", 1, T - 1, (self.B,), salt=38 + self.rank + self.world * idx)
            pos = torch.arange(T).view(1, T)
            ids = torch.where(pos == 0, torch.full_like(ids, 101), ids)
            ids = torch.where(pos == (n.view(-1, 1) + 1), torch.full_like(ids, 102), ids)
            ids = torch.where(pos > (n.view(-1, 1) + 1), torch.zeros_like(ids), ids)
            b["decoder_tokens"] = ids.to(self.device)
        return b

    def train_batches(self, epoch):
        n = max(math.ceil(math.ceil(self.train_samples / self.world) / self.B), 1)   # == plan()'s micro_per_epoch
        for i in range(n):
            yield self.pool[(epoch * n + i) % len(self.pool)]

    def val_batches(self):
        n = max(self.val_samples // (self.B * self.world), 1)
        for i in range(n):
            yield self.val_pool[i % len(self.val_pool)]


def vqa_score(logits, targets):
    """VQAScore.update (my_metrics.py:66-79): one-hot of the arg-max logit against the soft targets."""
    idx = logits.float().argmax(dim=1)
    return targets.float().gather(1, idx.view(-1, 1)).sum(), logits.shape[0]


def state_dict_cpu(model):
    return {k: v.detach().to("cpu", copy=True) for k, v in model.state_dict().items()}


class Trainer:
    def __init__(self, cfg, model, dm, rank=0, world=1, device="cuda", log_every=10):
        self.cfg, self.model, self.dm, self.rank, self.world, self.device = cfg, model, dm, rank, world, device
        self.store = model.store
        self.reducer = FlatGradReducer(self.store)
        self.plan = plan(cfg, world, dm.train_samples)
        if cfg["decay_power"] != "cosine" and not isinstance(cfg["decay_power"], (int, float)):
            raise ValueError(f"decay_power must be a number or 'cosine' (m3ae_utils.py:225), got {cfg['decay_power']!r}")
        # the reference's ([optimizer], [{"scheduler", "interval": "step"}]) (m3ae_utils.py:240-242), driven as Lightning drives it
        self.max_steps = self.plan["max_steps"]
        model.trainer_ref = self
        opts, scheds = model.configure_optimizers()
        self.optimizer, self.scheduler = opts[0], scheds[0]["scheduler"]
        self.global_step, self.epoch, self.best = 0, 0, -1.0
        self.log_every = log_every
        exp = cfg["exp_name"]
        run_name = f'{exp}-seed{cfg["seed"]}-from_{str(cfg["load_path"]).replace("/", "_")}'  # main.py:31
        self.ckpt_dir = os.path.join(cfg["log_dir"], run_name, "checkpoints")
        self.weights_only = "finetune" in exp  # main.py:42
        self.history = []
        # config key `vqa_metrics`: "host" (the overall score in ATen) | "device" (m3ae_amd/metrics.py: overall / closed / open / @k,
        # and token exact match in test() for the generator heads).  metrics / exact_match: the result() dicts of the last pass.
        self.vqa_metrics = config_mod.vqa_metrics(cfg)
        self.metrics, self.exact_match = None, None
        # config key `answer_decoding`: "free" | "list" (test() with vqa_metrics="device" and a generator head also decodes on
        # `answer_trie`, an answer_trie.AnswerTrie: set_answer_list or assign it).  answer_metrics: its result() dict of the last pass.
        self.answer_decoding = config_mod.answer_decoding(cfg)
        self.answer_trie, self.answer_metrics, self.answer_k = None, None, 1
        # config keys `answer_beams` / `answer_length_penalty` (read under "list" only): 1 = the greedy list search; 2 .. 8 = the
        # constrained beam search (csrc/trie_beam.hip), whose min(eval_topk, answer_beams) best labels per row give the `@k` score
        self.answer_beams, self.answer_length_penalty = config_mod.answer_beams(cfg)
        # config key `answer_scoring` (read under "list" only): "search" = the list search above; "exhaustive" = every entry scored in
        # one tree-shaped decoder pass (Decoder.answer_scores_async), min(eval_topk, 16, A) best labels for `@k`, and `answer_mass`,
        # the mean probability the head puts on the list; answer_beams is then ignored
        self.answer_scoring = config_mod.answer_scoring(cfg)
        self.answer_mass = None
        # config key `pretrain_metrics`: "host" (nothing beyond the monitored loss) | "device" (metrics.PretrainMetrics);
        # pretrain: its result() dict of the last pass
        self.pretrain_metrics = config_mod.pretrain_metrics(cfg)
        self.pretrain = None
        self.ema_eval = config_mod.ema_decay(cfg) > 0 and cfg.get("ema_eval", True)
        if getattr(self.store, "lora", None) is not None:
            log(self.store.lora.describe(), rank)
        self.validated_on_ema = False    # whether the last validate() ran on the averaged weights

    # -- checkpoints (reference key names; loadable by m3ae_module.py:105-113 upstream) ------------------------
    def save(self, name, metric=None):
        if self.rank != 0:
            return None
        os.makedirs(self.ckpt_dir, exist_ok=True)
        ck = {"state_dict": state_dict_cpu(self.model), "global_step": self.global_step, "epoch": self.epoch,
              "hyper_parameters": {"config": {k: v for k, v in self.cfg.items()}}, "val/the_metric": metric}
        if self.metrics is not None:
            ck["val/closed_score"], ck["val/open_score"] = self.metrics["closed"], self.metrics["open"]
        if self.pretrain:
            for name in ("mlm", "itm"):
                if name in self.pretrain:
                    ck[f"val/{name}_accuracy"] = self.pretrain[name]["accuracy"]
            for name in ("mlm", "itm", "mim"):
                if f"{name}_loss" in self.pretrain:
                    ck[f"val/{name}_loss"] = self.pretrain[f"{name}_loss"]
        if self.store.ema is not None:   # ema_decay > 0: the average next to the raw weights, in weights-only checkpoints too
            ck["ema_state_dict"], ck["ema_updates"] = self.store.ema_state_dict(), self.store.ema_updates
        lora = getattr(self.store, "lora", None)
        if lora is not None:   # lora_rank > 0: state_dict above holds the merged weights; the adapters (+ heads) next to them
            ck["lora_state_dict"] = lora.state_dict()
            if not self.weights_only:
                ck["lora_optimizer_state"] = lora.optimizer_state()
        if not self.weights_only:   # Lightning's keys
            ck["optimizer_states"] = [self.optimizer.state_dict()]
            ck["lr_schedulers"] = [self.scheduler.state_dict()]
        path = os.path.join(self.ckpt_dir, name)
        torch.save(ck, path)
        if lora is not None:   # the adapter-only file: base checkpoint + this = the fine-tuned model (config key lora_path)
            torch.save(ck["lora_state_dict"], os.path.splitext(path)[0] + ".lora.pt")
        return path

    def resume(self, path):
        ck = torch.load(path, map_location="cpu", weights_only=False)
        self.model.load_state_dict(ck["state_dict"], strict=False)
        self.store.sync_shadows()
        lora = getattr(self.store, "lora", None)
        if lora is not None:
            # the adapters go back onto the base taken from load_path at attach time (the fingerprint says whether it is the base they
            # were trained on) and are merged again: the same bits state_dict held
            if ck.get("lora_state_dict") is None:
                raise ValueError(f"{path} has no lora_state_dict: it was not written by a run with lora_rank > 0")
            lora.load_state_dict(ck["lora_state_dict"])
            lora.load_optimizer_state(ck.get("lora_optimizer_state"))
        self.global_step, self.epoch = ck.get("global_step", 0), ck.get("epoch", 0)
        if ck.get("ema_state_dict") is not None and self.store.ema_decay > 0:
            self.store.load_ema_state_dict(ck["ema_state_dict"], ck.get("ema_updates", 0))
        elif self.store.ema_decay > 0:
            self.store.ema, self.store.ema_updates = None, 0
            self.store._alloc_ema()
            log(f"{path} has no ema_state_dict: the average starts from the loaded weights", self.rank)
        of = ck.get("optimizer_flat")   # checkpoints written before the Optimizer face existed
        if ck.get("optimizer_states"):
            self.optimizer.load_state_dict(ck["optimizer_states"][0])    # state of another optim_type: ValueError
            self.scheduler.load_state_dict(ck["lr_schedulers"][0])
            if self.store.optim == "sgd":    # torch's SGD state carries no step count
                self.store.step_count = self.global_step
        elif of is not None and of["exp_avg"] is not None:
            if self.store.optim != "adamw":
                raise ValueError(f'{path}: AdamW moments (optimizer_flat) cannot resume a run with optim_type="{self.store.optim}"')
            self.store.exp_avg = of["exp_avg"].to(self.device)
            self.store.exp_avg_sq = of["exp_avg_sq"].to(self.device)
            self.store.step_count = of["step_count"]
        if not ck.get("optimizer_states"):
            if of is None:
                self.store.step_count = self.global_step
            self.scheduler.last_epoch = self.store.step_count   # LambdaLR: lr = base * lambda(last_epoch)
            for g, base in zip(self.optimizer.param_groups, self.scheduler.base_lrs):
                g["lr"] = base * self.store.lr_factor(self.store.step_count, self.max_steps)
        return ck

    # -- loops ------------------------------------------------------------------------------------------------
    def _loss(self, batch):
        out = self.model.training_step(batch)
        return out["loss"] if isinstance(out, dict) else out

    def _generator_metric(self):
        """TokenExactMatch for the generator head of the model with its pad / start / end ids as the skip set, and the function
        batch -> reference token ids; (None, None) for the classification model."""
        m = self.model
        if hasattr(m, "tokens_of"):       # decoder head: [CLS] answer [SEP] [PAD]...
            return metrics_mod.TokenExactMatch((m.pad_id, m.cls_id, m.sep_id), self.device), m.tokens_of
        if hasattr(m, "labels_of"):       # T5 head: answer </s> <pad>...
            c = m.t5.config
            return metrics_mod.TokenExactMatch((c.pad_token_id, c.decoder_start_token_id, c.eos_token_id), self.device), m.labels_of
        return None, None

    def set_answer_list(self, label2ans):
        """Builds `answer_trie` for answer_decoding="list" from the data set's answer list through the model's tokenizer: label2ans
        is the reference's mapping with string keys ("0" .. str(n - 1)) or a list of answers; entry i becomes label i.  The
        decoder head's sequences end in [SEP], the T5 head's in </s>."""
        from .answer_trie import AnswerTrie
        m = self.model
        tok = getattr(m, "tokenizer", None)
        if tok is None or not (hasattr(m, "tokens_of") or hasattr(m, "labels_of")):
            raise ValueError("set_answer_list needs a generator head constructed with a tokenizer; assign trainer.answer_trie otherwise")
        answers = [label2ans[str(i)] for i in range(len(label2ans))] if isinstance(label2ans, dict) else list(label2ans)
        end = m.sep_id if hasattr(m, "tokens_of") else m.t5.config.eos_token_id
        ids = []
        for a in answers:
            t = [int(v) for v in tok(a, add_special_tokens=False).input_ids]
            ids.append(t[:-1] if t and t[-1] == end else t)
        self.answer_trie = AnswerTrie.from_answers(ids, end)
        return self.answer_trie

    def answer_text(self):
        """` answer_list X (n) closed Y (n) open Z (n)` of the last test pass ("" unless answer_decoding="list" ran), with
        ` @k W` after a pass with answer_beams > 1 and k = min(eval_topk, answer_beams) > 1."""
        r = self.answer_metrics
        if r is None:
            return ""
        text = f" answer_list {r['score']:.4f} ({r['n']}) closed {r['closed']:.4f} ({r['n_closed']}) open {r['open']:.4f} ({r['n_open']})"
        if self.answer_k > 1:   # the beam form fed its n-best labels: the best target among a row's k best answers
            text += f" @{self.answer_k} {r['score_at_k']:.4f}"
        if self.answer_mass is not None:   # answer_scoring="exhaustive": `@k` always, then the mean of exp(log_mass)
            if self.answer_k <= 1:
                text += f" @1 {r['score']:.4f}"
            text += f" mass {self.answer_mass:.4f}"
        return text

    def pretrain_text(self):
        """`mlm acc X (n) @k Y ppl Z | itm acc X (n) | mim loss X` of the last pass ("" with pretrain_metrics="host")."""
        r = self.pretrain
        if not r:
            return ""
        parts = []
        if "mlm" in r:
            m = r["mlm"]
            parts.append(f"mlm acc {m['accuracy']:.4f} ({m['n']}) @{self.cfg.get('eval_topk', 5)} {m['accuracy_at_k']:.4f} ppl {m['perplexity']:.4g}")
        if "itm" in r:
            parts.append(f"itm acc {r['itm']['accuracy']:.4f} ({r['itm']['n']})")
        if "mim_loss" in r:
            parts.append(f"mim loss {r['mim_loss']:.4f}")
        return " " + " | ".join(parts) if parts else ""

    def metrics_text(self):
        """The closed / open / @k part of the validation log line ("" with vqa_metrics="host"), then the pre-training part
        ("" with pretrain_metrics="host")."""
        r = self.metrics
        if r is None:
            return self.pretrain_text()
        return self.pretrain_text() + f" closed {r['closed']:.4f} ({r['n_closed']}) open {r['open']:.4f} ({r['n_open']}) @{self.cfg.get('eval_topk', 5)} {r['score_at_k']:.4f}"

    def validate(self, generate=False):
        """The monitored quantity over the validation batches.  generate (test() with vqa_metrics="device"): the generator heads
        also run their device-resident search per batch and feed TokenExactMatch from the ids, which stay on the device.
        With ema_decay > 0, `ema_eval` and an average to read, the whole pass runs inside ParamStore.ema_weights()."""
        self.validated_on_ema = bool(self.ema_eval and self.store.ema is not None)
        if self.validated_on_ema:
            with self.store.ema_weights():
                return self._validate(generate)
        return self._validate(generate)

    def _validate(self, generate):
        self.model.eval()
        tot, cnt = torch.zeros((), device=self.device), 0
        device_metrics = self.vqa_metrics == "device"
        score = metrics_mod.VQARADScore(self.device, k=self.cfg.get("eval_topk", 5)) if device_metrics and hasattr(self.model, "vqa_head_forward") else None
        em, refs_of = self._generator_metric() if device_metrics and generate else (None, None)
        ans = ans_err = None    # answer_decoding="list": the generator head's answers as labels, scored like the classification head's
        if em is not None and self.answer_decoding == "list":
            if self.answer_trie is None:
                raise ValueError('answer_decoding="list" needs trainer.answer_trie: call set_answer_list(label2ans) or assign an AnswerTrie')
            self.answer_k = max(min(int(self.cfg.get("eval_topk", 5)), self.answer_beams), 1) if self.answer_beams > 1 else 1
            exhaustive, self.answer_mass = self.answer_scoring == "exhaustive", None
            if exhaustive:
                if not hasattr(self.model, "answer_scores_async"):
                    raise ValueError('answer_scoring="exhaustive" needs a generator head with answer_scores_async')
                self.answer_k = max(min(int(self.cfg.get("eval_topk", 5)), ops.LIST_MAX_K, self.answer_trie.num_answers), 1)
                mass = torch.zeros((2,), dtype=torch.float64, device=self.device)     # sum of exp(log_mass), samples
                if self.answer_beams > 1:
                    log(f'answer_scoring="exhaustive": answer_beams={self.answer_beams} is ignored', self.rank)
            ans = metrics_mod.VQARADScore(self.device, k=self.answer_k if self.answer_k > 1 else 0)
            ans_err = torch.zeros((1,), dtype=torch.int64, device=self.device)
        pre = None     # pretrain_metrics="device": built at the first batch that brings a pre-training objective
        fed = 0
        with torch.no_grad():
            for batch in self.dm.val_batches():
                n = batch["text_ids"].shape[0]
                ret = None
                if hasattr(self.model, "vqa_head_forward"):
                    self.model.set_task()
                    ret = self.model(batch, test=True)
                if ret is not None and "vqa_logits" in ret and score is not None:
                    score.update(ret["vqa_logits"], ret["vqa_targets"], batch.get("answer_types"))   # enqueued; read once below
                    fed += 1
                    continue
                if ret is not None and "vqa_logits" in ret:
                    s, n = vqa_score(ret["vqa_logits"], ret["vqa_targets"])
                elif ret is not None:   # pre-training objectives: negative summed loss as the monitored quantity
                    if self.pretrain_metrics == "device" and any(k in ret for k in ("mlm_logits", "itm_logits", "mim_loss")):
                        if pre is None:
                            pre = metrics_mod.PretrainMetrics(self.device, k=self.cfg.get("eval_topk", 5))
                        pre.update(ret)          # enqueued; read once below
                    s = -sum(v.float() for k, v in ret.items() if k.endswith("_loss")) * n
                else:                   # generator heads: negative teacher-forced loss
                    s = -self._loss(batch).float() * n
                    if em is not None:
                        em.update(self.model.generate_async(batch).seq, refs_of(batch), batch.get("answer_types"))
                    if ans is not None:     # enqueued; read once below
                        if exhaustive:
                            r = self.model.answer_scores_async(batch, self.answer_trie, self.answer_k, self.answer_length_penalty)
                            labels = r.labels if self.answer_k > 1 else r.label
                            mass[0] += torch.exp(r.log_mass).sum()
                            mass[1] += n
                        elif self.answer_beams > 1:
                            r = self.model.answer_async(batch, self.answer_trie, num_beams=self.answer_beams,
                                                        length_penalty=self.answer_length_penalty)
                            labels = r.labels[:, :self.answer_k] if self.answer_k > 1 else r.label
                        else:
                            r = self.model.answer_async(batch, self.answer_trie)
                            labels = r.label
                        ans_err += r.err
                        ans.update_labels(labels, build_vqa_targets(batch, self.cfg["vqa_label_size"], self.device), batch.get("answer_types"))
                tot += s
                cnt += n
        self.model.train()
        if em is not None:
            self.exact_match = em.result()
        if ans is not None:
            self.answer_metrics = ans.result()
            if getattr(ans, "label_err", None) is not None:
                ans_err += ans.label_err
            if exhaustive:      # the error word and the mass in the one blocking copy
                if self.world > 1:
                    dist.all_reduce(mass)
                both = torch.cat([ans_err.to(torch.float64), mass]).cpu()
                self.answer_mass = float(both[1] / both[2]) if float(both[2]) > 0 else None
                bad = float(both[0]) != 0
            else:
                bad = int(ans_err.cpu()) != 0
            if bad:
                raise ops._lib.M3AEHipError("answer-list decoding: a row left the answer table, or a label is outside [0, vqa_label_size)")
        if pre is not None:
            self.pretrain = pre.result()     # one all-reduce and one blocking copy for all of them
        if fed:
            self.metrics = score.result()    # the record's all-reduce and its one blocking copy
            return self.metrics["score"]
        t = torch.stack([tot, torch.tensor(float(cnt), device=self.device)])
        if self.world > 1:
            dist.all_reduce(t)
        return (t[0] / t[1]).item()

    def fit(self):
        """The training loop, issued on the library's high-priority launch stream (ops.launch_stream: the image half's kernels are
        dispatched ahead of the text half's on the side stream); the caller's stream is current again when it returns."""
        if not torch.cuda.is_available():
            return self._fit()
        prev = ops.use_launch_stream()
        try:
            # config key `deterministic` (the reference trainer's deterministic=True, main.py:64): ordered reductions for the run
            with ops.deterministic_mode(ops.deterministic() or bool(self.cfg.get("deterministic", False))):
                return self._fit()
        finally:
            torch.cuda.synchronize()
            torch.cuda.set_stream(prev)

    def _fit(self):
        P, cfg = self.plan, self.cfg
        gs = P["grad_steps"]
        self.model.train()
        ops.set_dropout_seed(cfg["seed"] * 1000003 + self.rank)
        vci = cfg["val_check_interval"]
        val_every = max(int(P["micro_per_epoch"] * vci), 1) if isinstance(vci, float) else int(vci)
        log(f"fit: world {self.world}, per-GPU batch {cfg['per_gpu_batchsize']}, grad_steps {gs}, "
            f"{P['steps_per_epoch']} optimizer steps/epoch, max_steps {P['max_steps']}", self.rank)
        t0, seen = time.perf_counter(), 0
        done = self.global_step >= P["max_steps"]
        while not done and self.epoch < P["max_epochs"]:
            micro, nbatch = 0, 0   # position inside the accumulation window / batches of this epoch
            it = iter(self.dm.train_batches(self.epoch))
            nxt = next(it, None)
            while nxt is not None:
                batch, nxt = nxt, next(it, None)
                # a window ends after grad_steps micro-batches -- or with the epoch (Lightning steps on the last batch)
                first, last = micro % gs == 0, (micro % gs == gs - 1 or nxt is None)
                if first:
                    self.optimizer.zero_grad()
                # exchange gradients only on the window's last micro-batch (Lightning skips the DDP sync otherwise)
                (self.reducer.attach() if last else self.reducer.detach())
                loss = self._loss(batch) / gs
                loss.backward()
                micro = 0 if last else micro + 1
                nbatch += 1
                seen += cfg["per_gpu_batchsize"] * self.world
                if last:
                    self.reducer.finish()
                    self.optimizer.grad_scale = self.reducer.grad_scale
                    self.optimizer.step()
                    self.scheduler.step()
                    self.global_step += 1
                    if self.global_step % self.log_every == 0 or self.global_step == 1:
                        lv = loss.item() * gs
                        dt = time.perf_counter() - t0
                        self.history.append((self.global_step, lv))
                        clip = ""
                        if self.store.clip_val() > 0:   # loss.item() above has synced: the record of this step is complete
                            gs_ = self.store.grad_stats()
                            clip = f" grad_norm {gs_['norm']:.4g} coef {gs_['coef']:.4f} skipped {gs_['skipped_steps']}"
                        log(f"epoch {self.epoch} step {self.global_step}/{P['max_steps']} loss {lv:.4f} "
                            f"lr x{self.store.lr_factor(self.store.step_count, P['max_steps']):.4f} "
                            f"{seen / dt:.1f} pairs/s{clip}", self.rank)
                    if self.global_step >= P["max_steps"]:
                        done = True
                if nbatch % val_every == 0 or done:
                    m = self.validate()
                    log(f"val/the_metric{' (ema)' if self.validated_on_ema else ''} {m:.4f} (best {max(self.best, m):.4f}){self.metrics_text()}", self.rank)
                    if m > self.best:
                        self.best = m
                        self.save("best.ckpt", m)
                    self.save("last.ckpt", m)
                if done:
                    break
            self.epoch += 1
        self.reducer.detach()
        return {"global_step": self.global_step, "best": self.best, "history": self.history}

    def test(self):
        m = self.validate(generate=True)
        em = ""
        if self.exact_match is not None:
            r = self.exact_match
            em = f" token_exact_match {r['score']:.4f} ({r['n']}) closed {r['closed']:.4f} ({r['n_closed']}) open {r['open']:.4f} ({r['n_open']})"
        log(f"test/the_metric{' (ema)' if self.validated_on_ema else ''} {m:.4f}{self.metrics_text()}{em}{self.answer_text()}", self.rank)
        return m


def init_distributed():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        from .ddp import rccl_group_options
        dist.init_process_group("nccl", device_id=dev, pg_options=rccl_group_options())  # nccl == RCCL on ROCm; its streams at the launch stream's priority
    return rank, world, dev


def build_model(cfg, head, device):
    from .modules import DecoderModel, M3AETransformerSS, T5VQA_MMEncoderInput
    lora_rank = config_mod.lora_rank(cfg)
    if lora_rank > 0 and head in ("t5", "decoder"):
        raise ValueError(f"lora_rank > 0 is not available with the {head} head: its M3AE is frozen and produces no weight gradient "
                         "to project")
    if head == "t5":
        model = T5VQA_MMEncoderInput(cfg)
        model.unfreeze_top_layers(cfg["unfreeze_num_encoder_layers"], cfg["unfreeze_num_decoder_layers"])
    elif head == "decoder":
        model = DecoderModel(cfg)
    else:
        model = M3AETransformerSS(cfg)
    lp = cfg["load_path"]
    if lp and os.path.exists(lp):
        target = model.m3ae if head in ("t5", "decoder") else model
        target._load(lp)  # m3ae_module.py:104-113: ckpt["state_dict"], strict=False, pos-embed resize
    else:
        # no checkpoint on disk (offline box): deterministic random init of the named architecture
        synth.fill_deterministic(model)
    mode = cfg.get("compute_dtype", "bf16")
    model.finalize(device, mode if mode in ("bf16", "fp32", "fp32x3") else torch.float32)
    if lora_rank > 0:   # after finalize and load_path: the weights as they stand are the base; then lora_path, then the merge
        model.attach_lora(cfg.get("lora_path", ""))
    return model


def run(argv, head="cls", tokenizer=None):
    """Entry point shared by main.py / main_t5_m3ae.py / main_decoder_m3ae.py: `python main.py with k=v ...
    named_config ...`.  `tokenizer`: optional callable for the arrow pipeline (default: the `tokenizer=` directory)."""
    cfg = config_mod.parse_cli(argv)
    rank, world, dev = init_distributed()
    expect = (cfg["num_gpus"] if isinstance(cfg["num_gpus"], int) else len(cfg["num_gpus"])) * cfg["num_nodes"]
    if expect != world:
        raise SystemExit(f"num_gpus * num_nodes = {expect} but the launcher started {world} process(es): start one "
                         f"process per GPU with `python -m torch.distributed.run --nproc-per-node {expect} ...`")
    if cfg["per_gpu_batchsize"] <= 0:
        raise SystemExit("per_gpu_batchsize must be set (run_scripts/*.sh pass it explicitly)")
    if cfg.get("image_dedup") and any(cfg["loss_names"].get(k, 0) > 0 for k in ("mim", "itm")):
        raise SystemExit("image_dedup=True cannot be combined with the mim / itm objectives: they read the image pixels per "
                         "sample (loss_names: " + ", ".join(k for k, v in cfg["loss_names"].items() if v > 0) + ")")
    torch.manual_seed(cfg["seed"])  # pl.seed_everything (main.py:19)
    root = cfg["data_root"]
    model = build_model(cfg, head, dev)
    if root in ("", "synthetic"):
        dm = SyntheticDataModule(cfg, rank, world, dev, head=head)
    else:
        from .data import ArrowDataModule  # arrow reader + CLIP transform + collate, prefetched
        if head != "cls" and getattr(model, "tokenizer", None) is None:
            raise SystemExit("the generator heads need their answer tokenizer (T5 / BERT vocabulary files) for real data: "
                             "construct the model with `tokenizer=` or use data_root=synthetic")
        dm = ArrowDataModule(cfg, rank, world, dev, tokenizer=tokenizer, head=head)
    tr = Trainer(cfg, model, dm, rank, world, dev)
    if cfg.get("resume_from"):
        tr.resume(cfg["resume_from"])
    out = {}
    if not cfg["test_only"]:
        out = tr.fit()
        if world > 1:
            dist.barrier()  # rank 0 has written best.ckpt
        if "finetune" in cfg["exp_name"] and os.path.exists(os.path.join(tr.ckpt_dir, "best.ckpt")):
            step = tr.global_step
            tr.resume(os.path.join(tr.ckpt_dir, "best.ckpt"))  # trainer.test(ckpt_path="best") (main.py:80)
            tr.global_step = out["global_step"] = step
    out["test"] = tr.test()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({k: v for k, v in out.items() if k != "history"}))
    return out
