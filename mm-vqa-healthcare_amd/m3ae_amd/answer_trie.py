"""The prefix trie of a list of candidate answers, for answer-list decoding of the generator heads (csrc/answer_trie.hip;
Decoder.answer_path_async, T5.constrained_greedy_async).  numpy only; torch is imported by `to_device` alone.

Entry i of the list is label i.  The trie is stored as CSR arrays, all int32:
  child_off  [N + 1]  the children of node n are entries child_off[n] .. child_off[n + 1] - 1
  child_tok  [E]      the token of an entry, ascending within a node
  child_node [E]      the node behind it
  leaf_label [N]      the label at the node behind an end token, -1 elsewhere
Node 0 is the root; nodes are numbered in breadth-first order and children in ascending token order, so the arrays are a function of
the list alone.  Every sequence ends with an end token and holds none before, so a leaf has no child and every other node has one:
a row of the search cannot get stuck.  The device follows the table unchecked (as lora.LoraTable): `to_device` is the check."""
import numpy as np


class AnswerTrie:
    def __init__(self, sequences, end_ids):
        end_ids = (int(end_ids),) if np.isscalar(end_ids) else tuple(int(e) for e in end_ids)
        seqs = [tuple(int(t) for t in s) for s in sequences]
        if not seqs:
            raise ValueError("AnswerTrie: the answer list is empty")
        seen = {}
        for i, s in enumerate(seqs):
            if any(t < 0 for t in s):
                raise ValueError(f"AnswerTrie: answer {i} holds a negative token id")
            if not s or s[-1] not in end_ids:
                raise ValueError(f"AnswerTrie: answer {i} does not end with an end token {end_ids}")
            if any(t in end_ids for t in s[:-1]):
                raise ValueError(f"AnswerTrie: answer {i} holds an end token before its last position")
            if s in seen:
                raise ValueError(f"AnswerTrie: answers {seen[s]} and {i} are the same token sequence")
            seen[s] = i
        self.end_ids, self.sequences = end_ids, seqs
        self.num_answers = len(seqs)
        self.depth = max(len(s) for s in seqs)
        # breadth-first: a node is the set of answers that share a prefix; its children split that set by the next token
        child_off, child_tok, child_node, leaf_label = [0], [], [], [-1]
        queue = [(list(range(len(seqs))), 0)]      # (answers through the node, its depth), in node order
        head = 0
        while head < len(queue):
            members, d = queue[head]
            head += 1
            groups = {}
            for i in members:
                if len(seqs[i]) > d:
                    groups.setdefault(seqs[i][d], []).append(i)
            for tok in sorted(groups):
                g = groups[tok]
                child_tok.append(tok)
                child_node.append(len(queue))
                # behind an end token stands exactly one answer (no end token inside, no duplicates)
                leaf_label.append(g[0] if tok in end_ids else -1)
                queue.append((g, d + 1))
            child_off.append(len(child_tok))
        self.child_off = np.asarray(child_off, dtype=np.int32)
        self.child_tok = np.asarray(child_tok, dtype=np.int32)
        self.child_node = np.asarray(child_node, dtype=np.int32)
        self.leaf_label = np.asarray(leaf_label, dtype=np.int32)
        self.num_nodes, self.num_edges = len(leaf_label), len(child_tok)
        self.max_token = int(self.child_tok.max())
        self._uploaded = {}             # device -> the int32 trie buffer
        self._uploaded_answers = {}     # (device, max_len, pad_id) -> the int64 answers table

    @classmethod
    def from_answers(cls, id_lists, end_id):
        """The trie of answers given without their end token: `end_id` is appended to each."""
        return cls([list(s) + [int(end_id)] for s in id_lists], (int(end_id),))

    def children(self, node):
        """(tokens, nodes) of a node's children."""
        lo, hi = int(self.child_off[node]), int(self.child_off[node + 1])
        return self.child_tok[lo:hi], self.child_node[lo:hi]

    def walk(self, seq):
        """The node reached from the root along `seq`, or -1 when the trie has no such path."""
        n = 0
        for t in seq:
            toks, nodes = self.children(n)
            j = int(np.searchsorted(toks, t))
            if j >= len(toks) or toks[j] != t:
                return -1
            n = int(nodes[j])
        return n

    def answers_table(self, max_len, pad_id):
        """The answers as a pad-filled int64 [A, max_len] array, row i = label i with its end token."""
        tab = np.full((self.num_answers, max_len), int(pad_id), dtype=np.int64)
        for i, s in enumerate(self.sequences):
            tab[i, :len(s)] = s
        return tab

    def to_device(self, device, V, max_len, pad_id=None):
        """Uploads the arrays as one int32 buffer and returns a namespace of views of it (child_off, child_tok, child_node,
        leaf_label, buf, N, E, A, depth).  ValueError if a token is >= V or the longest answer exceeds max_len: the kernels follow
        the table as it is.  With `pad_id` the namespace also holds `answers`, the upload of answers_table(max_len, pad_id) (the
        beam search reads the token row of its best label from it)."""
        import torch
        from types import SimpleNamespace as NS
        if self.max_token >= V:
            raise ValueError(f"AnswerTrie: token {self.max_token} is outside a vocabulary of {V}")
        if self.depth > max_len:
            raise ValueError(f"AnswerTrie: the longest answer has {self.depth} tokens, the search has room for {max_len}")
        N, E = self.num_nodes, self.num_edges
        device = torch.device(device)
        buf = self._uploaded.get(device)
        if buf is None:             # one upload per device; from pinned memory, so that the copy does not make the host wait
            host = torch.from_numpy(np.concatenate([self.child_off, self.child_tok, self.child_node, self.leaf_label]))
            buf = host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host
            self._uploaded[device] = buf
        o1, o2, o3 = N + 1, N + 1 + E, N + 1 + 2 * E
        ns = NS(child_off=buf[:o1], child_tok=buf[o1:o2], child_node=buf[o2:o3], leaf_label=buf[o3:], buf=buf, N=N, E=E,
                A=self.num_answers, depth=self.depth)
        if pad_id is not None:
            key = (device, int(max_len), int(pad_id))
            tab = self._uploaded_answers.get(key)
            if tab is None:
                host = torch.from_numpy(self.answers_table(max_len, pad_id))
                tab = host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host
                self._uploaded_answers[key] = tab
            ns.answers = tab
        return ns
