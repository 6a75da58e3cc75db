"""Service — the backend object the MCP tools and the CLI talk to; same signatures and defaults
as the reference (reference src/lean_explore/search/service.py:15-68: limit=20, rerank_top=50)."""

from __future__ import annotations

import time

from .engine import SearchEngine
from .types import SearchResponse, SearchResult


class Service:
    def __init__(self, engine: SearchEngine | None = None):
        # reference service.py:21: no engine -> the default one (cache paths from the environment)
        self.engine = engine or SearchEngine()

    async def search(self, query: str, limit: int = 20, rerank_top: int | None = 50,
                     packages: list[str] | None = None, *,
                     prefilter_packages: bool = False, prefilter_lexical: bool = False) -> SearchResponse:
        if prefilter_lexical and not prefilter_packages:
            raise ValueError("prefilter_lexical=True needs prefilter_packages=True: the flag means 'prefilter both stages'")
        start = time.time()
        if prefilter_packages and packages:  # the dense stage searches only the packages' rows
            if prefilter_lexical:  # ... and the lexical stage only the packages' names
                results = await self.engine.search_prefiltered(query=query, packages=packages, limit=limit,
                                                               rerank_top=rerank_top, lexical=True)
            else:
                results = await self.engine.search_prefiltered(query=query, packages=packages, limit=limit,
                                                               rerank_top=rerank_top)
        else:
            results = await self.engine.search(query=query, limit=limit, rerank_top=rerank_top,
                                               packages=packages)
        return SearchResponse(query=query, results=results, count=len(results),
                              processing_time_ms=int((time.time() - start) * 1000))

    async def get_by_id(self, declaration_id: int) -> SearchResult | None:
        return await self.engine.get_by_id(declaration_id)
