"""Data source of the retrieval hot path — host-side mirror of reference ragroute/data_source.py.

Same class and method names (`DataSource.retrieve_docs_medrag/fed4rag/wikipedia(query_embed, k)`,
`load_faiss_index`, `run_data_source`) and the same return tuples, but `index.search` is the HIP flat
scan over an HBM-resident corpus (flat_index.FlatIndex).  Row -> id -> text lookups stay on the host
exactly as data_source.py:143-215 does them.  Beyond the reference's single-query call shape, every
`retrieve_docs_*` accepts a [B,d] batch and then returns one tuple per query."""
import json
import logging
import os
import time

import numpy as np

from . import config
from .flat_index import FlatIndex, normalize_L2

logger = logging.getLogger("client")


_FLAT_FOURCC = {b"IxFI": 0, b"IxF2": 1}   # IndexFlatIP -> METRIC_INNER_PRODUCT, IndexFlatL2 -> METRIC_L2


def read_faiss_flat_index(path, mmap=True):
    """Minimal reader for a FAISS IndexFlat file: returns (float32 [ntotal,d], "ip" | "l2") — what `faiss.read_index`
    (data_source.py:71) yields for the flat indexes the scan kernel replaces.
    With mmap=True (default) the payload is memory-mapped, so a 70 GB index (MedRAG pubmed: 23.9 M x 768 f32) is streamed
    into HBM chunk by chunk by FlatIndex.add instead of being loaded into host RAM first.

    Layout (FAISS 1.7.x impl/index_write.cpp, `write_index_header` + the IndexFlat branch; little endian):
        fourcc        4 B   "IxFI" (inner product) | "IxF2" (L2) | "IxFl" (IndexFlat with another metric)
        d             i32
        ntotal        i64
        dummy, dummy  2 x i64 (1 << 20)
        is_trained    u8
        metric_type   i32   0 = METRIC_INNER_PRODUCT, 1 = METRIC_L2, > 1 = other metrics, followed by
        [metric_arg   f32   only when metric_type > 1]
        size          u64   payload length in 4-byte units (= ntotal * d)
        payload       size x f32, row-major
    Anything else — a non-flat index (HNSW, IVF, PQ ...), a metric other than IP / L2, a header that contradicts its
    fourcc or its payload — raises ValueError, which the service loop logs (data_source.py:137-138).
    The layout is external knowledge (faiss is not in the reference tree nor in this image): byte-level fixtures in
    tests/test_faiss_file_format.py restate it independently of the writer below."""
    with open(path, "rb") as f:
        head = f.read(4 + 4 + 8 + 16 + 1 + 4)
        if len(head) < 4:
            raise ValueError(f"{path}: not a FAISS index file (shorter than a fourcc)")
        fourcc = head[:4]
        if fourcc not in _FLAT_FOURCC and fourcc != b"IxFl":
            raise ValueError(f"{path}: not a flat FAISS index (fourcc {fourcc!r}); only IndexFlatIP / IndexFlatL2 files are supported")
        if len(head) < 37:
            raise ValueError(f"{path}: truncated IndexFlat header")
        d = int(np.frombuffer(head, np.int32, 1, 4)[0])
        ntotal = int(np.frombuffer(head, np.int64, 1, 8)[0])
        metric_type = int(np.frombuffer(head, np.int32, 1, 33)[0])
        if metric_type not in (0, 1):
            raise ValueError(f"{path}: metric_type {metric_type} is not supported (only 0 = inner product and 1 = L2)")
        if fourcc in _FLAT_FOURCC and _FLAT_FOURCC[fourcc] != metric_type:
            raise ValueError(f"{path}: fourcc {fourcc!r} contradicts metric_type {metric_type}")
        if d <= 0 or ntotal < 0:
            raise ValueError(f"{path}: bad header (d={d}, ntotal={ntotal})")
        size = f.read(8)
        if len(size) < 8:
            raise ValueError(f"{path}: truncated IndexFlat header")
        nfloat = int(np.frombuffer(size, np.uint64)[0])
        if nfloat != ntotal * d:
            raise ValueError(f"{path}: payload of {nfloat} floats does not match ntotal*d = {ntotal * d}")
        offset = f.tell()
        f.seek(0, 2)
        if f.tell() - offset < nfloat * 4:
            raise ValueError(f"{path}: file holds {f.tell() - offset} payload bytes, header promises {nfloat * 4}")
        f.seek(offset)
        if mmap and ntotal > 0:
            xb = np.memmap(path, dtype=np.float32, mode="r", offset=offset, shape=(ntotal, d))
        else:
            xb = np.fromfile(f, dtype=np.float32, count=nfloat).reshape(ntotal, d)
    return xb, ("ip" if metric_type == 0 else "l2")


def write_faiss_flat_index(path, xb, metric="ip"):
    """Writer of the same layout (test fixtures / synthetic corpora)."""
    xb = np.ascontiguousarray(xb, np.float32)
    with open(path, "wb") as f:
        f.write(b"IxFI" if metric == "ip" else b"IxF2")
        f.write(np.int32(xb.shape[1]).tobytes())
        f.write(np.int64(xb.shape[0]).tobytes())
        f.write(np.int64(1 << 20).tobytes() * 2)
        f.write(np.uint8(1).tobytes())
        f.write(np.int32(0 if metric == "ip" else 1).tobytes())
        f.write(np.uint64(xb.size).tobytes())
        xb.tofile(f)


class MedragMetadata:
    """`metadatas.jsonl` (data_source.py:73: one {"index": int, "source": str} object per corpus row, consumed at 169-170) as two
    columns instead of one Python dict per row: pubmed's 23.9 M rows are 0.2 GB of numpy instead of ~6 GB of dicts, and a window's
    nq x k lookups are two fancy-index calls.  Behaves like the reference's list for what the path does with it: len(), [row] ->
    {"index", "source"} (a fresh dict with the same content); `take(rows)` is the batched form."""

    def __init__(self, index, source_code, sources):
        self.index = np.asarray(index, np.int64)
        self.source_code = np.asarray(source_code, np.int32)
        self.sources = list(sources)
        self._names = np.empty(len(self.sources), dtype=object)
        self._names[:] = self.sources

    @classmethod
    def from_jsonl(cls, path):
        """Returns a MedragMetadata, or the plain list of dicts if a line carries anything but exactly {"index", "source"}.
        The file is streamed (pubmed's has 23.9 M lines): the lines are those of `file.read().strip().split("\\n")`
        (data_source.py:73) - blank lines at the ends are dropped, a blank line in the middle fails in json.loads as it does there."""
        from array import array
        index, code, names, lookup, plain = array("q"), array("i"), [], {}, None
        pending_blank = 0
        started = False
        with open(path, "r") as f:
            for raw in f:
                line = raw.rstrip("\n")
                if not line.strip():
                    if started:
                        pending_blank += 1          # only an error if a non-blank line follows
                    continue
                if not started:
                    line = line.lstrip()            # .strip() of the whole text removes leading whitespace of the first line ...
                    started = True
                if pending_blank:
                    json.loads("")                  # the reference would be parsing an empty line here: same JSONDecodeError
                m = json.loads(line)
                if plain is None and (not isinstance(m, dict) or len(m) != 2 or type(m.get("index")) is not int or not isinstance(m.get("source"), str)):
                    plain = [{"index": int(i), "source": names[c]} for i, c in zip(index, code)]
                if plain is not None:
                    plain.append(m)
                    continue
                c = lookup.get(m["source"])
                if c is None:
                    c = lookup[m["source"]] = len(names)
                    names.append(m["source"])
                index.append(m["index"])
                code.append(c)
        if not started:
            json.loads("")                          # an empty file: `"".split("\\n")` is [""], which the reference fails to parse
        if plain is not None:
            return plain
        return cls(np.frombuffer(index, np.int64) if len(index) else np.zeros(0, np.int64),
                   np.frombuffer(code, np.int32) if len(code) else np.zeros(0, np.int32), names)

    def __len__(self):
        return len(self.index)

    def __getitem__(self, row):
        return {"index": int(self.index[row]), "source": self.sources[self.source_code[row]]}

    def take(self, rows):
        """rows: int array -> (list of index ints, list of source names, int64 array of keys source_code << 40 | index), one
        entry per row; everything is a numpy gather."""
        rows = np.asarray(rows, np.int64)
        idx, code = self.index[rows], self.source_code[rows]
        return idx.tolist(), self._names[code].tolist(), (code.astype(np.int64) << 40) | idx


class JsonlLines:
    """The lines of a chunk file as the reference indexes them (`file.read().strip().split("\\n")`, data_source.py:173-176), kept
    as ONE bytes object plus the line offsets, found once: [i] -> the bytes of line i (json.loads takes bytes)."""

    def __init__(self, path):
        with open(path, "rb") as f:
            buf = f.read()
        begin = len(buf) - len(buf.lstrip())
        end = len(buf.rstrip())
        self.buf = buf
        nl = np.flatnonzero(np.frombuffer(buf, np.uint8, end - begin, begin) == 10).astype(np.int64) + begin
        self.starts = np.concatenate([[begin], nl + 1])
        self.ends = np.concatenate([nl, [end]])
        if end == begin:     # "".split("\n") == [""]: one empty line, as the reference's list would hold
            self.starts, self.ends = np.array([begin]), np.array([begin])

    def __len__(self):
        return len(self.starts)

    def __getitem__(self, i):
        if i < 0:
            i += len(self.starts)
        return self.buf[self.starts[i]: self.ends[i]]


def open_jsonl_lines(path):
    """JsonlLines, or — where byte-wise and text-mode reading would index differently (carriage returns: text mode translates
    them; non-ASCII or \\x1c-\\x1f whitespace at the file's ends: str.strip() removes more than bytes.strip()) — the reference's own list."""
    lines = JsonlLines(path)
    buf = lines.buf
    edge = [buf[lines.starts[0]], buf[lines.ends[-1] - 1]] if lines.ends[-1] > lines.starts[0] else []
    if b"\r" in buf or any(c >= 0x80 or 0x1c <= c <= 0x1f for c in edge):
        with open(path, "r") as f:
            return f.read().strip().split("\n")
    return lines


def _take(seq, rows):
    """[seq[i] for i in rows] at C speed."""
    if not rows:
        return []
    if len(rows) == 1:
        return [seq[rows[0]]]
    from operator import itemgetter
    return list(itemgetter(*rows)(seq))


class DataSource:
    def __init__(self, client_id: int, dataset: str, name: str, simulate: bool = False, dtype: str = "fp16"):
        self.client_id = client_id
        self.dataset = dataset
        self.simulate = simulate
        self.dtype = dtype
        if dataset == "medrag":
            self.dataset_dir = config.MEDRAG_DIR
        elif dataset == "feb4rag":
            self.dataset_dir = config.FEB4RAG_DIR
        elif dataset == "wikipedia":
            self.dataset_dir = config.WIKIPEDIA_DIR
        else:
            raise ValueError(f"Unknown dataset when starting data source {name}: {dataset}")
        self.name = name
        self.recv_port = config.SERVER_CLIENT_BASE_PORT + client_id
        self.send_port = config.CLIENT_SERVER_BASE_PORT + client_id
        self.running = False
        if dataset == "medrag":
            self.index_dir = os.path.join(self.dataset_dir, name, "index", "ncbi/MedCPT-Article-Encoder")
            self.index_path = os.path.join(self.index_dir, "faiss.index")
            self.doc_ids_path = os.path.join(self.index_dir, "metadatas.jsonl")
        elif dataset == "feb4rag":
            self.index_dir = os.path.join(self.dataset_dir, "dataset_creation", "2_search", "embeddings", name)
            model_name = config.EMBEDDING_MODELS_PER_DATA_SOURCE[dataset][name][0]
            self.index_path = os.path.join(self.index_dir, f"{name}_{model_name}.faiss")
            self.doc_ids_path = os.path.join(self.index_dir, f"{name}_{model_name}.docids.json")
        else:
            self.index_dir = os.path.join(self.dataset_dir, "faiss_clusters", "normalized_indexes")
            self.index_path = os.path.join(self.index_dir, f"faiss_index_{name}_normalized.index")
            self.doc_ids_path = None
        self.mmlu_titles, self.mmlu_texts = [], []
        self.faiss_indexes = None
        self.cache_jsonl = {}
        self._parsed_docs = {}
        self._docs_by_key = {}
        self._batcher = None
        self.batch_window_ms = float(os.environ.get("RAGROUTE_BATCH_WINDOW_MS", 0.2))
        # RAGROUTE_EXACT_F32=1: keep the index file's f32 rows beside the half copy and return the reference's f32 results
        # (FlatIndex exact_f32, or exact_l2 where the index file's metric is L2; 3x the half bytes of HBM)
        self.exact_f32 = os.environ.get("RAGROUTE_EXACT_F32", "0") not in ("", "0")

    # -- loading (data_source.py:69-80) -------------------------------------------------------------
    def load_faiss_index(self):
        logger.info(f"Loading FAISS index for {self.name}")
        xb, file_metric = read_faiss_flat_index(self.index_path)
        self.index_metric = file_metric  # the index FILE decides the metric in the reference (faiss.read_index, data_source.py:71)
        if self.dataset == "medrag":
            metadatas = MedragMetadata.from_jsonl(self.doc_ids_path)
        elif self.dataset == "feb4rag":
            with open(self.doc_ids_path, "r") as f:
                metadatas = json.load(f)
        else:
            metadatas = []
            split = os.path.join(self.dataset_dir, "faiss_clusters", "split_texts_titles")
            with open(os.path.join(split, f"titles_{self.name}.txt"), "r", encoding="utf-8") as f:
                self.mmlu_titles = f.read().splitlines()
            with open(os.path.join(split, f"texts_{self.name}.txt"), "r", encoding="utf-8") as f:
                self.mmlu_texts = f.read().splitlines()
        self.set_index(xb, metadatas)

    def pick_device(self):
        """The GPU this data-source PROCESS keeps its corpus on.  The reference starts one process per source (ragroute.py:10-16)
        and knows no devices; on a multi-GPU node the drop-in spreads those processes over the visible GPUs: `RAGROUTE_DEVICE`
        (an index or "cuda:i") if set, else `client_id mod device_count` - SURVEY 8e's source s -> GPU s mod G for the module
        surface (the device-side pipeline balances by row slices instead: placement.py).  None = the current device."""
        import torch
        env = os.environ.get("RAGROUTE_DEVICE")
        if env:
            return torch.device(env if ":" in env else f"cuda:{int(env)}")
        n = torch.cuda.device_count()
        return torch.device(f"cuda:{self.client_id % n}") if n > 1 else None

    def set_index(self, xb, metadatas, titles=None, texts=None):
        """Install a corpus directly: xb float32 [n,d] (numpy / memmap) or an existing FlatIndex."""
        if isinstance(xb, FlatIndex):
            index = xb
        else:
            metric = getattr(self, "index_metric", "ip")
            kw = {"exact_l2" if metric == "l2" else "exact_f32": True} if self.exact_f32 else {}
            index = FlatIndex(xb.shape[1], metric=metric, dtype=self.dtype, device=self.pick_device(), **kw)
            index.reserve(xb.shape[0])
            index.add(xb)
        self.faiss_indexes = index, metadatas
        if titles is not None:
            self.mmlu_titles, self.mmlu_texts = list(titles), list(texts)

    # -- retrieval (data_source.py:143-215) -----------------------------------------------------------
    def _search(self, query_embed, k):
        q = np.asarray(query_embed, dtype=np.float32)
        single = q.ndim == 1 or q.shape[0] == 1
        q = q.reshape(1, -1) if q.ndim == 1 else q
        index, metadatas = self.faiss_indexes
        D, I = index.search(q, k)
        return D, I, metadatas, single

    def _chunk_lines(self, source):
        lines = self.cache_jsonl.get(source)
        if lines is None:
            lines = self.cache_jsonl[source] = open_jsonl_lines(os.path.join(self.dataset_dir, self.name, "chunk", f"{source}.jsonl"))
        return lines

    def _medrag_idx2txt(self, indices):
        """data_source.py:166-183: the JSONL line `index` of chunk/{source}.jsonl, parsed.  Each line is parsed on first touch and
        kept (the reference re-parses it on every hit); like the reference's FeB4RAG corpus entries (data_source.py:144-155) the
        parsed objects are shared between replies — callers serialise them, nobody mutates them."""
        results = []
        for i in indices:
            source, index = i["source"], i["index"]
            parsed = self._parsed_docs.setdefault(source, {})
            doc = parsed.get(index)
            if doc is None:
                doc = parsed[index] = json.loads(self._chunk_lines(source)[index])
            results.append(doc)
        return results

    # Reply building, batched: (D f32 [nq,k], I i64 [nq,k]) -> one (ids, docs, scores) tuple per query, the reference's tuples
    # (data_source.py:163, 194, 215).  One pass over the window's nq x k candidates: the id -> metadata -> text lookups are array
    # gathers and C-level list gathers, not per-candidate Python loops.
    def _replies_medrag(self, D, I):
        _, metadatas = self.faiss_indexes
        valid = I >= 0
        counts = valid.sum(1).tolist()
        rows = I[valid]
        if isinstance(metadatas, MedragMetadata):
            idx, src, keys = metadatas.take(rows)
            metas = [{"index": i, "source": s_} for i, s_ in zip(idx, src)]
            # texts: one C-level pass over the window through a cache keyed by (source, index); lines parsed on first touch
            cache = self._docs_by_key
            docs = list(map(cache.get, keys.tolist()))
            if None in docs:
                for j, doc in enumerate(docs):
                    if doc is None:
                        docs[j] = cache[int(keys[j])] = self._medrag_idx2txt((metas[j],))[0]
        else:
            metas = _take(metadatas, rows.tolist())
            docs = self._medrag_idx2txt(metas)
        scores = D.tolist()
        out, pos, k = [], 0, I.shape[1]
        for q, c in enumerate(counts):
            out.append((metas[pos: pos + c], docs[pos: pos + c], scores[q] if c == k else scores[q][:c]))
            pos += c
        return out

    def _feb4rag_corpus(self):
        if self.name not in self.cache_jsonl:
            corpus = {}
            path = os.path.join(self.dataset_dir, "dataset_creation/original_dataset", self.name, self.name, "corpus.jsonl")
            with open(path, "r") as file:
                for line in file:
                    entry = json.loads(line)
                    corpus[entry["_id"]] = entry
            self.cache_jsonl[self.name] = corpus
        return self.cache_jsonl[self.name]

    def _replies_fed4rag(self, D, I):
        _, docids = self.faiss_indexes
        corpus_data = self._feb4rag_corpus()
        valid = I >= 0
        counts = valid.sum(1).tolist()
        ids = _take(docids, I[valid].tolist())
        docs = [corpus_data.get(doc_id, None) for doc_id in ids]
        out, pos = [], 0
        for c in counts:
            out.append((ids[pos: pos + c], docs[pos: pos + c], []))      # no scores for FeB4RAG (data_source.py:163)
            pos += c
        return out

    def _replies_wikipedia(self, D, I):
        valid = I >= 0
        counts = valid.sum(1).tolist()
        rows = I[valid].tolist()
        docs = list(zip(_take(self.mmlu_titles, rows), _take(self.mmlu_texts, rows)))
        scores = D.tolist()
        out, pos = [], 0
        for q, c in enumerate(counts):
            out.append((rows[pos: pos + c], docs[pos: pos + c], scores[q][:c]))
            pos += c
        return out

    def retrieve_docs_medrag(self, query_embed, k):
        D, I, _, single = self._search(query_embed, k)
        out = self._replies_medrag(D, I)
        return out[0] if single else out

    def retrieve_docs_fed4rag(self, query_embed, k):
        D, I, _, single = self._search(query_embed, k)
        out = self._replies_fed4rag(D, I)
        return out[0] if single else out

    def retrieve_docs_wikipedia(self, query_embed, k):
        query_vec = np.ascontiguousarray(np.asarray(query_embed, dtype=np.float32).reshape(-1, np.asarray(query_embed).shape[-1]))
        normalize_L2(query_vec)  # data_source.py:198-199
        D, I, _, single = self._search(query_vec, k)
        out = self._replies_wikipedia(D, I)
        return out[0] if single else out

    # -- batched serving ---------------------------------------------------------------
    @staticmethod
    def tune_runtime():
        """Process-level settings of a data-source SERVICE process (called by start(); a library user decides for itself): the
        loaded corpus metadata, texts and caches are moved out of the garbage collector's generations (gc.freeze) and the
        generation-0 threshold is raised.  A window of 256 replies allocates ~17 k small containers; at CPython's default
        thresholds that is ~25 young collections and regular full ones per window, each walking whatever replies are alive —
        measured: reply building 25.7 -> 10.9 us per request (profiles/r04/service_throughput.json)."""
        import gc
        gc.collect()
        gc.freeze()
        gc.set_threshold(100_000, 50, 100)

    def search_batch(self, embeddings, k=None):
        """Stage 1 of a window (the batcher's SEARCH thread): decode the embeddings, ONE GPU search (+ the wikipedia sources'
        normalize_L2, data_source.py:198-199), copy-out.  Returns the handle build_replies() takes."""
        k = config.K[self.dataset] if k is None else k
        batch = np.stack([np.asarray(e, dtype=np.float32).reshape(-1) for e in embeddings])
        if self.dataset == "wikipedia":
            batch = np.ascontiguousarray(batch)
            normalize_L2(batch)
        index, _ = self.faiss_indexes
        return index.search(batch, k)

    def build_replies(self, handle):
        """Stage 2 of a window (the batcher's REPLY thread, overlapping the next window's search): one (ids, docs, scores) tuple
        per query."""
        D, I = handle
        return {"medrag": self._replies_medrag, "feb4rag": self._replies_fed4rag, "wikipedia": self._replies_wikipedia}[self.dataset](D, I)

    def retrieve_batch(self, embeddings, k=None):
        """One GPU search for a window of queries; returns one (ids, docs, scores) tuple per query."""
        return self.build_replies(self.search_batch(embeddings, k))

    async def handle_query(self, query_data):
        """Reply message for one request, in the reference's wire format (data_source.py:123-131).  Concurrent
        requests are coalesced by the batcher into one scan of up to 256 queries."""
        import asyncio
        start_time = time.time()
        if self.simulate:
            ids, docs, scores = ["doc1", "doc2", "doc3"], ["Document 1 content", "Document 2 content", "Document 3 content"], [0.9, 0.85, 0.8]
            await asyncio.sleep(config.DATA_SOURCE_DELAY)
        else:
            if self._batcher is None:
                from .queue_manager import QueryBatcher
                self._batcher = QueryBatcher(search=self.search_batch, finish=self.build_replies, max_batch=256, max_wait_ms=self.batch_window_ms)
            ids, docs, scores = await self._batcher.enqueue(query_data["embedding"])
        return {"query_id": query_data["id"], "client_id": self.client_id, "name": self.name, "indices": ids, "docs": docs,
                "scores": scores, "duration": time.time() - start_time}

    # -- service loop (transport glue; needs pyzmq like the reference) ----------------------------------
    async def start(self):
        """data_source.py:82-141: bind PULL :6000+i, connect PUSH :7500+i, load the index, then serve.  Every request
        becomes its own task so that requests arriving together meet in the batcher (one scan for the window)."""
        import asyncio
        import zmq
        import zmq.asyncio
        self.context = zmq.asyncio.Context()
        self.running = True
        self.receiver = self.context.socket(zmq.PULL)
        self.receiver.bind(f"tcp://*:{self.recv_port}")
        self.sender = self.context.socket(zmq.PUSH)
        self.sender.connect(f"tcp://localhost:{self.send_port}")
        self._serve_task = asyncio.current_task()
        pending = set()
        try:
            if not self.simulate and self.faiss_indexes is None:
                self.load_faiss_index()
            if not self.simulate:
                self.tune_runtime()

            async def reply(query_data):
                try:
                    await self.sender.send_json(await self.handle_query(query_data))
                except asyncio.CancelledError:
                    raise
                except Exception as e:  # logged, reply dropped — as data_source.py:137-138
                    logger.error(f"Error when fetching documents from data source {self.name} (query data: {query_data}): {e}")

            while self.running:
                query_data = await self.receiver.recv_json()
                task = asyncio.ensure_future(reply(query_data))
                pending.add(task)
                task.add_done_callback(pending.discard)
        except asyncio.CancelledError:
            logger.info(f"Client {self.client_id} shutdown requested")
        finally:
            for task in list(pending):
                task.cancel()
            self.stop()

    def stop(self):
        """Stop serving and close the sockets (data_source.py:217-222)."""
        self.running = False
        task, self._serve_task = getattr(self, "_serve_task", None), None
        batcher = self._batcher
        if batcher is not None:
            batcher.shutdown_threads()       # the search / reply threads of the two-stage batcher end with the service
        for name in ("receiver", "sender"):
            sock = getattr(self, name, None)
            if sock is not None:
                sock.close()
                setattr(self, name, None)
        ctx = getattr(self, "context", None)
        if ctx is not None:
            ctx.term()
            self.context = None
        if task is not None and not task.done():
            import asyncio
            try:
                current = asyncio.current_task()
            except RuntimeError:
                current = None
            if task is not current:
                task.cancel()


CURRENT = {}   # client_id -> the DataSource this process serves with (set by run_data_source; introspection / tests)


async def run_data_source(client_id: int, dataset: str, name: str, simulate: bool = False):
    """Process entry with the reference's signature (data_source.py:224-226)."""
    CURRENT[client_id] = data_source = DataSource(client_id, dataset, name, simulate=simulate)
    await data_source.start()
