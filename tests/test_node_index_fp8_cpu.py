"""gpu_service node mode with ``INDEX_DTYPE=fp8`` on CPU gloo ranks: the ``/index/*`` endpoints and the rank-local
ingest write and search FP8 shards; results must equal a single-process FP8 ``VectorIndex`` (the search is exact
over the quantised rows)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytest.importorskip("fastapi")

W = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _entry(rank, world, port, out_path):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), GPU_SERVICE_DEVICE="cpu", INDEX_DTYPE="fp8")
    torch.set_num_threads(1)
    from django_assistant_bot_amd.parallel.node import NodePlan
    from gpu_service import node_main

    node = node_main.setup(embedders=["tiny-bert"], providers=[], plan=NodePlan(world), backend="gloo",
                           device_type="cpu")
    try:
        if rank == 0:
            _drive(node, out_path)
        else:
            node.follow()
    finally:
        node_main.teardown(node)


def _drive(node, out_path):
    from fastapi import FastAPI
    from fastapi.testclient import TestClient

    from django_assistant_bot_amd.engine.vector_index import VectorIndex
    from gpu_service import main as svc

    app = FastAPI()
    for r in svc.app.routes:
        app.router.routes.append(r)
    c = TestClient(app)
    res = {}
    # ---- upsert (the second overwrites some ids), filtered search, delete
    g = torch.Generator().manual_seed(4)
    dim = 16
    ids = np.arange(1, 401) * 5
    vecs = torch.randn(400, dim, generator=g)
    docs, groups = ids // 20, (ids // 5) % 2
    c.post("/index/q/upsert", json={"ids": ids[:250].tolist(), "vectors": vecs[:250].tolist(),
                                    "doc_ids": docs[:250].tolist(), "groups": groups[:250].tolist()})
    r2 = c.post("/index/q/upsert", json={"ids": ids[200:].tolist(), "vectors": vecs[200:].tolist(),
                                         "doc_ids": docs[200:].tolist(), "groups": groups[200:].tolist()})
    res["count"] = r2.json()["count"]
    res["shard_fp8"] = bool(node.indexes["q"].local.fp8)
    res["shard_bytes_per_row"] = node.indexes["q"].local.vecs.element_size() * dim + 1
    single = VectorIndex(dim, "cpu", dtype="fp8")
    single.add(ids, vecs, doc_ids=docs, groups=groups)
    q = torch.randn(5, dim, generator=g)
    body = {"queries": q.tolist(), "k": 30, "groups": [0, 1, 0, 1, 0],
            "allowed": [ids[::3].tolist()] * 5, "doc_lt": [int(docs[300])] * 5}
    got = c.post("/index/q/search", json=body).json()
    es, eids, edocs = single.search(q, 30, q_groups=body["groups"], allowed=body["allowed"], doc_lt=body["doc_lt"])
    res["search_equal"] = got["ids"] == [[x for x in row if x >= 0] for row in eids.tolist()]
    res["dist_err"] = max(abs((1 - s) - d) for srow, drow in zip(es.tolist(), got["distances"])
                          for s, d in zip(srow, drow))
    res["removed"] = c.post("/index/q/delete", json={"ids": ids[:10].tolist()}).json()["removed"]
    single.remove(ids[:10])
    got = c.post("/index/q/search", json={"queries": q.tolist(), "k": 8}).json()
    res["after_delete_equal"] = got["ids"] == single.search(q, 8)[1].tolist()
    # ---- ingest: every row is found by its own embedding
    n = 120
    tids = np.arange(n) * 7 + 2
    texts = [f"document {i} about topic {i % 13} and detail {i * 31 % 17}" for i in range(n)]
    r = c.post("/index/docs/ingest", json={"model": "tiny-bert", "ids": tids.tolist(), "texts": texts,
                                           "doc_ids": (tids // 10).tolist()})
    res["ingested"] = r.json()["count"]
    res["docs_fp8"] = bool(node.indexes["docs"].local.fp8)
    emb = node.embeds["tiny-bert"].embed(texts[::10], out_dtype=torch.float32).cpu()
    s = c.post("/index/docs/search", json={"queries": emb.tolist(), "k": 1}).json()
    res["top1"] = [x[0] for x in s["ids"]]
    res["want"] = tids[::10].tolist()
    torch.save(res, out_path)


def test_node_index_with_fp8_rows(tmp_path):
    out = str(tmp_path / "node.pt")
    mp.spawn(_entry, args=(W, _free_port(), out), nprocs=W, join=True)
    res = torch.load(out, weights_only=True)
    assert res["shard_fp8"] and res["docs_fp8"] and res["shard_bytes_per_row"] == 17
    assert res["count"] == 400
    assert res["search_equal"] and res["dist_err"] < 1e-4
    assert res["removed"] == 10 and res["after_delete_equal"]
    assert res["ingested"] == 120 and res["top1"] == res["want"]
