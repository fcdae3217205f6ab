// Batches with character classes or mismatch budgets (queries.cpp: vlg_queries_parse_classes, vlg_queries_set_mismatches) as stages.
// Part of search.hip's translation unit: included once from there, behind run_joins / read_stats.
#pragma once
namespace {
// Such a sub-pattern has a SET of pairwise disjoint SA intervals, one per member string, or string within the budget, that occurs
// (kernels.hip: branching_search_kernel).  Everything behind the occurrence lists sees a list as (L.off[s], occ[s]) only.  So distinct
// sub-patterns are found on the host by content and effective budget min(k, m), each is searched once (a literal one without a budget by
// backward_search_kernel: one interval), and per super-chunk the intervals of one are expanded back to back into ONE list, located by
// the random-access walks, sorted inside itself and joined by plan_joins / run_joins unchanged.
struct ClassBatch {
    const vlg_index* idx; const vlg_queries* q; vlg_workspace* ws; vlg_result* res; PhaseTrace& tr;
    hipStream_t st = ws->stream;
    const uint64_t nsub = q->nsub, n = idx->hdr.n;
    const uint32_t cap = ws->class_intervals;
    const bool wide = idx->hdr.sample_bytes == 8;   // 33-bit SA indices; the positions still fit 32 bits (n <= 2^32 + 1)
    // per sub-pattern its distinct id and effective budget; per distinct id the first sub-pattern of the batch that is it
    std::vector<uint32_t> sub_d; std::vector<uint8_t> sub_kb; std::vector<uint64_t> d_sub; uint64_t nd = 0;
    std::vector<uint32_t> lit, cls, apx;            // distinct ids: literal and class without a budget, either with one
    svec<uint8_t> lblob, arows; svec<uint64_t> loff, task; bool own_rows = false; uint64_t group = 1;     // what the searches read
    // the carve of the workspace's head buffer
    struct { unsigned long long* stats; uint8_t* lblob; uint64_t* loff; uint64_t* ll; uint64_t* lr; uint64_t* task; uint32_t* count; uint64_t* frontier; uint8_t* arows; } f{};
    std::vector<std::vector<uint64_t>> iv_l, iv_r;  // the searches: per distinct id its intervals, ascending
    Plan pl;
    static constexpr uint64_t kFixed = 8ull << 20;
    uint64_t budget = 0, phys_cap = 0; std::vector<uint32_t> stamp; uint32_t epoch = 0; Lists<uint32_t> L;

    bool literal(uint64_t s) const { return !q->has_classes() || q->sub_literal[s] != 0; }

    // distinct sub-patterns, by content and budget: literal ones by their bytes, the others by their mask rows
    vlg_status distinct()
    {
        const bool budgets = q->has_mismatches();
        sub_d.assign(nsub, 0); sub_kb.assign(nsub, 0);
        std::unordered_map<std::string, uint32_t> seen;
        seen.reserve(nsub * 2 + 16);
        std::string key;
        for (uint64_t s = 0; s < nsub; ++s) {
            const uint64_t a = q->suboff[s], b = q->suboff[s + 1];
            const uint64_t kb = budgets ? std::min<uint64_t>(q->sub_k[s], b - a) : 0;        // k >= m: every position may differ
            sub_kb[s] = (uint8_t)kb;
            if (literal(s)) { key.assign(1, 'L'); key.push_back((char)kb); key.append(reinterpret_cast<const char*>(q->blob.data() + a), b - a); }
            else { key.assign(1, 'C'); key.push_back((char)kb); key.append(reinterpret_cast<const char*>(q->masks.data() + a * 32), (b - a) * 32); }
            const auto it = seen.emplace(key, (uint32_t)d_sub.size());
            if (it.second) d_sub.push_back(s);
            sub_d[s] = it.first->second;
        }
        nd = d_sub.size();
        if (nd >= 0xFFFFFFF0ull) return fail(VLG_E_UNSUPPORTED, "too many distinct sub-patterns in one batch");
        for (uint32_t d = 0; d < nd; ++d) (sub_kb[d_sub[d]] ? apx : literal(d_sub[d]) ? lit : cls).push_back(d);
        iv_l.resize(nd); iv_r.resize(nd);
        return VLG_OK;
    }

    // the literal patterns back to back, the tasks of the branching searches (class sub-patterns, then the budgeted ones), the head buffer
    vlg_status stage_front()
    {
        const uint64_t nlit = lit.size(), ncls = cls.size(), napx = apx.size();
        loff.assign(nlit + 1, 0); task.assign(2 * std::max<uint64_t>(ncls + napx, 1), 0);
        for (uint64_t i = 0; i < nlit; ++i) {
            const uint64_t s = d_sub[lit[i]];
            lblob.insert(lblob.end(), q->blob.begin() + q->suboff[s], q->blob.begin() + q->suboff[s + 1]);
            loff[i + 1] = lblob.size();
        }
        for (uint64_t i = 0; i < ncls; ++i) { const uint64_t s = d_sub[cls[i]]; task[2 * i] = q->suboff[s]; task[2 * i + 1] = q->suboff[s + 1] - q->suboff[s]; }
        // a budgeted sub-pattern reads 256-bit rows: those of the batch, or -- a batch without classes has none -- rows made here, one bit each
        own_rows = napx && !q->has_classes();
        for (uint64_t i = 0; i < napx; ++i) {
            const uint64_t s = d_sub[apx[i]], a = q->suboff[s], m = q->suboff[s + 1] - a;
            task[2 * (ncls + i)] = own_rows ? arows.size() / 32 : a;
            task[2 * (ncls + i) + 1] = m | ((uint64_t)sub_kb[s] << 56);
            if (own_rows) {
                arows.resize(arows.size() + m * 32, 0);
                uint8_t* row = arows.data() + arows.size() - m * 32;
                for (uint64_t p = 0; p < m; ++p) { const uint8_t c = q->blob[a + p]; row[p * 32 + (c >> 3)] = (uint8_t)(1u << (c & 7)); }
            }
        }
        const uint64_t kClassScratch = 64ull << 20;                  // the frontiers of one group of tasks
        group = std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(std::max(ncls, napx), 1), kClassScratch / (32ull * cap)));
        // the head buffer: a pass over its parts without a base sizes it, a second one places them
        uint8_t* head = nullptr; uint64_t used = 0;
        const auto take = [&](auto*& p, uint64_t bytes) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(head + used); used += align_up(bytes, 256); };
        const auto carve = [&] {
            used = 0;
            take(f.stats, kStatsWords * 8);
            take(f.lblob, lblob.size() + 16);
            take(f.loff, (nlit + 1) * 8);
            take(f.ll, (nlit + 1) * 8);
            take(f.lr, (nlit + 1) * 8);
            take(f.task, 2 * (ncls + napx + 1) * 8);
            take(f.count, group * 4);
            take(f.frontier, 2 * group * cap * 16);
            take(f.arows, arows.size() + 32);
        };
        carve();
        if (vlg_status s = ws_head(ws, used, &head)) return s;
        carve();
        VLG_HIP_TRY(hipMemsetAsync(f.stats, 0, kStatsWords * 8, st));
        if (ncls + napx) VLG_HIP_TRY(hipMemcpyAsync(f.task, task.data(), 2 * (ncls + napx) * 8, hipMemcpyHostToDevice, st));
        if (own_rows) VLG_HIP_TRY(hipMemcpyAsync(f.arows, arows.data(), arows.size(), hipMemcpyHostToDevice, st));
        ws->sample_reads = 0;
        ws->x_agreed = 0;
        return VLG_OK;
    }

    // literal sub-patterns without a budget: one interval each
    vlg_status search_literals()
    {
        const uint64_t nlit = lit.size();
        if (!nlit) return VLG_OK;
        if (!lblob.empty()) VLG_HIP_TRY(hipMemcpyAsync(f.lblob, lblob.data(), lblob.size(), hipMemcpyHostToDevice, st));
        VLG_HIP_TRY(hipMemcpyAsync(f.loff, loff.data(), (nlit + 1) * 8, hipMemcpyHostToDevice, st));
        {
            Timed t(ws, KS_BSEARCH, 0);
            if (vlg_status s = launch_backward_search(idx->view, f.lblob, f.loff, nlit, f.ll, f.lr, f.stats + 3, st)) return s;
        }
        svec<uint64_t> hl(nlit), hr(nlit);
        VLG_HIP_TRY(hipMemcpyAsync(hl.data(), f.ll, nlit * 8, hipMemcpyDeviceToHost, st));
        VLG_HIP_TRY(hipMemcpyAsync(hr.data(), f.lr, nlit * 8, hipMemcpyDeviceToHost, st));
        VLG_HIP_TRY(hipStreamSynchronize(st));
        for (uint64_t i = 0; i < nlit; ++i)
            if (hr[i] + 1 > hl[i]) { iv_l[lit[i]].push_back(hl[i]); iv_r[lit[i]].push_back(hr[i]); }
        return VLG_OK;
    }

    // the branching searches of one kind, a group of tasks at a time: launch, count read-back, strided frontier copy
    vlg_status search_branching(const std::vector<uint32_t>& ids, const uint64_t* d_tk, const uint8_t* d_rows, bool with_budget)
    {
        const uint64_t nt = ids.size();
        if (!nt) return VLG_OK;
        svec<uint32_t> hc(group);
        svec<uint64_t> hf;
        for (uint64_t g0 = 0; g0 < nt; g0 += group) {
            const uint64_t g = std::min<uint64_t>(group, nt - g0);
            {
                Timed t(ws, KS_CLASS_SEARCH, 0);
                if (vlg_status s = launch_branching_search(idx->view, with_budget, d_rows, d_tk + 2 * g0, g, cap, f.frontier, f.count, f.stats + 3, st)) return s;
            }
            VLG_HIP_TRY(hipMemcpyAsync(hc.data(), f.count, g * 4, hipMemcpyDeviceToHost, st));
            VLG_HIP_TRY(hipStreamSynchronize(st));
            uint64_t widest = 0;
            for (uint64_t i = 0; i < g; ++i) {
                if (hc[i] == kClassSearchOverflow) {
                    // (nothing else is launched: the batch ends here)
                    const uint64_t s = d_sub[ids[g0 + i]];
                    const uint64_t qi = (uint64_t)(std::upper_bound(q->qsub.begin(), q->qsub.end(), s) - q->qsub.begin()) - 1;
                    return fail(VLG_E_WORKSPACE, "query " + std::to_string(qi) + ", sub-pattern " + std::to_string(s - q->qsub[qi]) + ": more than " +
                                                     std::to_string(cap) + " SA intervals at one step of its " + (with_budget ? "approximate" : "class") +
                                                     " search (workspace option \"class_intervals\")");
                }
                widest = std::max<uint64_t>(widest, hc[i]);
            }
            if (!widest) continue;
            // half 0 of the group's frontiers: `cap` intervals of 16 bytes per task, of which the first `widest` are fetched
            hf.resize(g * widest * 2);
            VLG_HIP_TRY(hipMemcpy2DAsync(hf.data(), widest * 16, f.frontier, (size_t)cap * 16, widest * 16, g, hipMemcpyDeviceToHost, st));
            VLG_HIP_TRY(hipStreamSynchronize(st));
            for (uint64_t i = 0; i < g; ++i) {
                const uint32_t d = ids[g0 + i];
                iv_l[d].reserve(hc[i]); iv_r[d].reserve(hc[i]);
                for (uint64_t j = 0; j < hc[i]; ++j) { iv_l[d].push_back(hf[(i * widest + j) * 2]); iv_r[d].push_back(hf[(i * widest + j) * 2 + 1]); }
            }
        }
        return VLG_OK;
    }

    // the Plan over the distinct sub-patterns, what vlg_result_class_intervals returns, the live queries, the physical budget
    vlg_status plan()
    {
        pl.occ.assign(nsub, 0);
        pl.did.assign(nsub, 0);
        pl.dl.assign(nd, 0);
        pl.docc.assign(nd, 0);
        for (uint64_t d = 0; d < nd; ++d) {
            for (size_t j = 0; j < iv_l[d].size(); ++j) pl.docc[d] += iv_r[d][j] + 1 - iv_l[d][j];
            pl.dl[d] = iv_l[d].empty() ? 0 : iv_l[d][0];
        }
        // per sub-pattern of the batch, the intervals of its distinct sub-pattern
        res->has_class_intervals = true;
        res->civ_off.assign(nsub + 1, 0);
        for (uint64_t s = 0; s < nsub; ++s) {
            res->civ_l.insert(res->civ_l.end(), iv_l[sub_d[s]].begin(), iv_l[sub_d[s]].end());
            res->civ_r.insert(res->civ_r.end(), iv_r[sub_d[s]].begin(), iv_r[sub_d[s]].end());
            res->civ_off[s + 1] = res->civ_l.size();
        }
        for (uint64_t qi = 0; qi < q->nq; ++qi) {
            if (!query_live(q, qi, [&](uint64_t s) { return pl.docc[sub_d[s]]; })) continue;
            for (uint64_t s = q->qsub[qi]; s < q->qsub[qi + 1]; ++s) { pl.did[s] = sub_d[s]; pl.occ[s] = pl.docc[sub_d[s]]; res->sum.logical_occurrences += pl.occ[s]; }
        }
        // super-chunks: whole queries while their distinct lists fit the physical budget (next_super_chunk, as the byte path)
        if (ws->cap_bytes <= 2 * kFixed) return fail(VLG_E_WORKSPACE, "workspace cap too small");
        budget = ws->cap_bytes - kFixed;
        phys_cap = std::min<uint64_t>(budget / 2 / (sizeof(uint32_t) + kSweepScratchPerElem + 1), 0xFFFFFF00ull);
        stamp.assign(nd, 0xFFFFFFFFu);
        L.doff.assign(nd, 0);
        L.off.assign(nsub, 0);
        return VLG_OK;
    }

    // the lists of one super-chunk, each the intervals of one distinct sub-pattern back to back
    struct ClassLists {
        ClassBatch& b; const SuperChunk& sc;
        uint64_t nl = 0, total = 0, niv = 0, n_long = 0, n_tiles = 0, n_chunks = 0;
        svec<uint64_t> off64, l, off;                   // the lists one after the other; the intervals each of them is made of
        ListRoom room{0, false};
        uint8_t* other = nullptr; uint64_t* d_off64 = nullptr; uint64_t* d_l = nullptr; uint64_t* d_off = nullptr; uint32_t* F = nullptr;
        ListSortPlan lp;

        vlg_status layout()
        {
            nl = sc.dlist.size();
            off64.assign(nl + 1, 0); off.assign(1, 0);
            for (uint64_t i = 0; i < nl; ++i) {
                const uint32_t d = sc.dlist[i];
                b.L.doff[d] = (uint32_t)off64[i];
                for (size_t j = 0; j < b.iv_l[d].size(); ++j) { l.push_back(b.iv_l[d][j]); off.push_back(off.back() + (b.iv_r[d][j] + 1 - b.iv_l[d][j])); }
                off64[i + 1] = off64[i] + b.pl.docc[d];
                const uint64_t len = b.pl.docc[d], t = (len + kSortTile - 1) / kSortTile;
                if (len > kSortTile) { ++n_long; n_tiles += t; n_chunks += (t + kSortChunk - 1) / kSortChunk; }
            }
            total = off64[nl]; niv = l.size();
            if (total != off.back() || total != sc.phys) return fail(VLG_E_INTERNAL, "class batch: list lengths disagree with their intervals");
            room = ListRoom(total, b.ws->filter);
            return VLG_OK;
        }
        uint64_t words() const { return total * (b.wide ? 8 : 4) + 8; }      // bytes of the walk / sort scratch
        // arena: [lists][room for the survivors of the window filter][walk / sort scratch][tables][fences] | filter state, join scratch
        uint64_t bytes() const
        {
            return align_up(room.positions() * 4, 256) + align_up(words(), 256) + align_up((nl + 1) * 8, 256) + align_up((niv + 1) * 8, 256) +
                   align_up((niv + 2) * 8, 256) + align_up(room.fence_entries * 4, 256) + align_up(nl * 4, 256) + kSortClasses * 256 +
                   list_sort_scratch_bytes(n_long, n_tiles, n_chunks) + 16 * 256 + 8192;
        }
        vlg_status carve(Arena& A)
        {
            b.L.P = A.take<uint32_t>(room.positions());
            other = A.take<uint8_t>(words());
            d_off64 = A.take<uint64_t>(nl + 1);
            d_l = A.take<uint64_t>(niv + 1);
            d_off = A.take<uint64_t>(niv + 2);
            F = A.take<uint32_t>(room.fence_entries);
            if (A.failed) return fail(VLG_E_INTERNAL, "arena carve failed (class lists)");
            if (!total) return VLG_OK;
            VLG_HIP_TRY(hipMemcpyAsync(d_off64, off64.data(), (nl + 1) * 8, hipMemcpyHostToDevice, b.st));
            VLG_HIP_TRY(hipMemcpyAsync(d_l, l.data(), niv * 8, hipMemcpyHostToDevice, b.st));
            VLG_HIP_TRY(hipMemcpyAsync(d_off, off.data(), (niv + 1) * 8, hipMemcpyHostToDevice, b.st));
            return list_sort_prepare(off64, (uint32_t)nl, A, b.st, lp, b.ws->sort_one_pass);
        }
        vlg_status locate()
        {
            if (!total) return VLG_OK;
            const IndexView lview = b.ws->quad_walk ? b.idx->view : without_quad(b.idx->view);
            if (vlg_status s = b.wide ? expand_and_walk(b.ws, lview, d_l, d_off, niv, total, reinterpret_cast<uint64_t*>(other), b.L.P, b.f.stats)
                                      : expand_and_walk(b.ws, lview, d_l, d_off, niv, total, b.L.P, b.L.P, b.f.stats)) return s;
            b.ws->sample_reads += total;
            b.res->sum.locate_mode = VLG_LOCATE_WALKS;
            return VLG_OK;
        }
        vlg_status sort()
        {
            if (!total) return VLG_OK;
            Timed t(b.ws, KS_SORT, 2ull * total * 4);
            return list_sort_enqueue(lp, b.L.P, reinterpret_cast<uint32_t*>(other), d_off64, std::max(1u, bit_width64(b.n >= 2 ? b.n - 2 : 0)), b.st, b.ws->list_sort != 2);
        }
        vlg_status fences() { return wire_room_and_fences(b.L, room, total, F, b.st); }
    };

    // one super-chunk from query Q0 on: its lists, then its joins; -> Q0 behind it
    vlg_status super_chunk(uint64_t& Q0)
    {
        SuperChunk sc;
        vlg_status s;
        if ((s = next_super_chunk(q, pl, false, phys_cap, Q0, stamp, epoch, sc))) return s;
        ClassLists cl{*this, sc};
        if ((s = cl.layout())) return s;
        const uint64_t list_bytes = cl.bytes();
        if (list_bytes >= budget) return fail(VLG_E_WORKSPACE, "the lists of a super-chunk do not fit the workspace cap");
        JoinPlan jp;
        if ((s = plan_joins(q, pl, ws, sc.Q0, sc.Q1, budget - list_bytes, n, jp))) return s;
        if ((s = ws_reserve(ws, list_bytes + jp.filter_need + jp.want_bytes + jp.meta + kFixed))) return s;
        Arena A{ws->arena, ws->arena_bytes};
        if ((s = cl.carve(A)) || (s = cl.locate()) || (s = cl.sort()) || (s = cl.fences())) return s;
        res->sum.located_occurrences += cl.total;
        tr.mark("class lists: locate + sort");
        for (uint64_t sp = q->qsub[sc.Q0]; sp < q->qsub[sc.Q1]; ++sp) L.off[sp] = pl.occ[sp] ? L.doff[pl.did[sp]] : 0;
        if ((s = run_joins<uint32_t>(n, q, ws, res, pl, L, A, sc.Q0, sc.Q1, jp, f.stats, tr))) return s;
        Q0 = sc.Q1;
        return VLG_OK;
    }
};

vlg_status run_class_batch(const vlg_index* idx, const vlg_queries* q, vlg_workspace* ws, vlg_result* res, PhaseTrace& tr)
{
    ClassBatch b{idx, q, ws, res, tr};
    vlg_status s;
    if ((s = b.distinct()) || (s = b.stage_front()) || (s = b.search_literals())) return s;
    if ((s = b.search_branching(b.cls, b.f.task, q->d_masks, false))) return s;
    if ((s = b.search_branching(b.apx, b.f.task + 2 * b.cls.size(), b.own_rows ? b.f.arows : q->d_masks, true))) return s;
    tr.mark("class search");
    if ((s = b.plan())) return s;
    for (uint64_t Q0 = 0; Q0 < q->nq;)
        if ((s = b.super_chunk(Q0))) return s;
    return read_stats(ws, res, b.f.stats, idx, KS_CLASS_SEARCH);
}

}  // namespace
