// The place-recognition entries of include/spslam_gpu.h: spslam_place_reloc_candidates[_batch_device]
// (KeyFrameDatabase::DetectRelocalizationCandidates), spslam_place_loop_candidates[_batch_device]
// (KeyFrameDatabase::DetectLoopCandidates) and spslam_place_min_score[_batch_device] (LoopClosing::DetectLoop's
// reference score).  The device forms trust their tables; the host forms check every index (place_check.h), stage
// one problem at base 0 and call the device forms.
#include "capi_ctx.h"
#include "place_check.h"
#include "place_launch.h"

namespace {

bool db_args_ok(const spslam_place_db* db) {
    return db && db->bow_words && db->bow_values && db->n_bow && db->in_db && db->cap >= 1 &&
           db->cap <= SPSLAM_PLACE_MAX_WORDS;
}

// One sequence's database on the device: slots 0 .. 4 of a host form's stage (words, values, n_bow, in_db, the
// score table the entry writes), the entry's own slots behind them from kFirst on.
struct DbStage {
    static constexpr int kScore = 4, kFirst = 5;
    const spslam_place_db& db;
    size_t K;
    float* score;  // host: reloc_score / loop_score, NULL: the entry reads none
    DbStage(const spslam_place_db& d, int n_kf, float* s) : db(d), K((size_t)n_kf), score(s) {}
    int open(Stage& st, std::initializer_list<StageSlot> entry_slots) const {
        const size_t W = K * (size_t)db.cap;
        std::vector<StageSlot> slots{{db.bow_words, W * 4}, {db.bow_values, W * 8}, {db.n_bow, K * 4}, {db.in_db, K},
                                     {score, score ? K * 4 : 0, K * 4}};
        slots.insert(slots.end(), entry_slots.begin(), entry_slots.end());
        return st.open(slots.data(), (int)slots.size());
    }
    spslam_place_db device(const Stage& st, bool loop) const {
        spslam_place_db d{};
        d.bow_words = st.slot<uint32_t>(0);
        d.bow_values = st.slot<double>(1);
        d.n_bow = st.slot<int>(2);
        d.in_db = st.slot<uint8_t>(3);
        (loop ? d.loop_score : d.reloc_score) = st.slot<float>(kScore);
        d.cap = db.cap;
        return d;
    }
};

// the result record, the candidates it counts and the score table back to the host
int fetch_candidates(spslam_ctx* c, Stage& st, int result_slot, int cand_slot, const DbStage& ds,
                     spslam_place_result* result, int32_t* candidates) {
    HIP_CHECK(c, hipMemcpyAsync(result, st.slot<void>(result_slot), sizeof *result, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(ds.score, st.slot<void>(DbStage::kScore), ds.K * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (result->n_candidates > 0)
        HIP_CHECK(c, hipMemcpy(candidates, st.slot<void>(cand_slot), (size_t)result->n_candidates * 4,
                               hipMemcpyDeviceToHost));
    return st.close();
}

}  // namespace

extern "C" {

int spslam_place_reloc_candidates_batch_device(spslam_ctx* c, int n_problems, const spslam_place_problem* d_problems,
                                               const spslam_place_db* db, const spslam_place_frames* frames,
                                               const spslam_covis_graph* graph, spslam_place_result* d_results,
                                               int32_t* d_candidates, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_problems < 1 || !d_problems || !db_args_ok(db) || !db->reloc_score || !frames || !frames->bow_words ||
        !frames->bow_values || !frames->n_bow || frames->cap < 1 || frames->cap > SPSLAM_PLACE_MAX_WORDS || !graph ||
        !graph->covis || !d_results || !d_candidates)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_place_reloc_candidates_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, place_reloc_launch(n_problems, d_problems, *db, *frames, *graph, d_results, d_candidates,
                                    (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_place_loop_candidates_batch_device(spslam_ctx* c, int n_problems, const spslam_place_problem* d_problems,
                                              const spslam_place_db* db, const spslam_covis_graph* graph,
                                              const float* d_min_score, spslam_place_result* d_results,
                                              int32_t* d_candidates, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_problems < 1 || !d_problems || !db_args_ok(db) || !db->loop_score || !graph || !graph->covis ||
        !graph->weights || graph->stride < 1 || !d_min_score || !d_results || !d_candidates)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_place_loop_candidates_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, place_loop_launch(n_problems, d_problems, *db, *graph, d_min_score, d_results, d_candidates,
                                   (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_place_min_score_batch_device(spslam_ctx* c, int n_problems, const spslam_place_problem* d_problems,
                                        const spslam_place_db* db, const spslam_covis_graph* graph,
                                        const uint8_t* d_kf_bad, float* d_min_score, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_problems < 1 || !d_problems || !db_args_ok(db) || !graph || !graph->ordered || !graph->n_ordered ||
        graph->stride < 1 || !d_min_score)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_place_min_score_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, place_min_score_launch(n_problems, d_problems, *db, *graph, d_kf_bad, d_min_score,
                                        (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_place_reloc_candidates(spslam_ctx* c, const spslam_place_db* db, int n_kf, const uint32_t* q_words,
                                  const double* q_values, int q_n, const spslam_covis_graph* graph,
                                  spslam_place_result* result, int32_t* candidates) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!db || !graph || !result || !candidates || !db->reloc_score)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_place_reloc_candidates");
    const char* e = place_check_db(*db, n_kf);
    if (!e) e = place_check_vector(q_words, q_values, q_n, SPSLAM_PLACE_MAX_WORDS);
    if (!e) e = place_check_covis(graph->covis, n_kf);
    if (e) return fail(c, SPSLAM_ERR_ARG, "spslam_place_reloc_candidates: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t K = (size_t)n_kf, Q = (size_t)q_n, QC = std::max(Q, (size_t)1);
    const spslam_place_problem P{0, n_kf, 0, 0};
    const DbStage ds(*db, n_kf, db->reloc_score);
    enum { kQWords = DbStage::kFirst, kQValues, kQN, kCovis, kProblem, kResult, kCand };
    Stage st(c);
    if (int rc = ds.open(st, {{q_words, Q * 4, QC * 4}, {q_values, Q * 8, QC * 8}, {&q_n, sizeof(int)},
                              {graph->covis, K * SPSLAM_COVIS_BEST * 4}, {&P, sizeof P}, sizeof(spslam_place_result),
                              K * 4}))
        return rc;
    const spslam_place_db dd = ds.device(st, false);
    spslam_place_frames df{};
    df.bow_words = st.slot<uint32_t>(kQWords);
    df.bow_values = st.slot<double>(kQValues);
    df.n_bow = st.slot<int>(kQN);
    df.cap = (int)QC;
    spslam_covis_graph dg{};
    dg.covis = st.slot<int32_t>(kCovis);
    int rc = spslam_place_reloc_candidates_batch_device(c, 1, st.slot<spslam_place_problem>(kProblem), &dd, &df, &dg,
                                                        st.slot<spslam_place_result>(kResult),
                                                        st.slot<int32_t>(kCand), c->stream);
    if (rc) return rc;
    return fetch_candidates(c, st, kResult, kCand, ds, result, candidates);
}

int spslam_place_loop_candidates(spslam_ctx* c, const spslam_place_db* db, int n_kf, int query,
                                 const spslam_covis_graph* graph, float min_score, spslam_place_result* result,
                                 int32_t* candidates) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!db || !graph || !result || !candidates || !db->loop_score || !graph->weights)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_place_loop_candidates");
    const char* e = place_check_db(*db, n_kf);
    if (!e) e = place_check_query(*graph, n_kf, query);
    if (!e) e = place_check_covis(graph->covis, n_kf);
    if (!e && db->in_db[query]) e = "the query keyframe is in the database";
    if (e) return fail(c, SPSLAM_ERR_ARG, "spslam_place_loop_candidates: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t K = (size_t)n_kf;
    const spslam_place_problem P{0, n_kf, query, 0};
    const DbStage ds(*db, n_kf, db->loop_score);
    enum { kCovis = DbStage::kFirst, kWeights, kMinScore, kProblem, kResult, kCand };
    Stage st(c);
    if (int rc = ds.open(st, {{graph->covis, K * SPSLAM_COVIS_BEST * 4}, {graph->weights, K * (size_t)graph->stride * 4},
                              {&min_score, sizeof(float)}, {&P, sizeof P}, sizeof(spslam_place_result), K * 4}))
        return rc;
    const spslam_place_db dd = ds.device(st, true);
    spslam_covis_graph dg{};
    dg.covis = st.slot<int32_t>(kCovis);
    dg.weights = st.slot<int32_t>(kWeights);
    dg.stride = graph->stride;
    int rc = spslam_place_loop_candidates_batch_device(c, 1, st.slot<spslam_place_problem>(kProblem), &dd, &dg,
                                                       st.slot<float>(kMinScore),
                                                       st.slot<spslam_place_result>(kResult), st.slot<int32_t>(kCand),
                                                       c->stream);
    if (rc) return rc;
    return fetch_candidates(c, st, kResult, kCand, ds, result, candidates);
}

int spslam_place_min_score(spslam_ctx* c, const spslam_place_db* db, int n_kf, int query,
                           const spslam_covis_graph* graph, const uint8_t* kf_bad, float* min_score) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!db || !graph || !min_score) return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_place_min_score");
    const char* e = place_check_db(*db, n_kf);
    if (!e) e = place_check_query(*graph, n_kf, query);
    if (!e) e = place_check_ordered(*graph, n_kf, query);
    if (e) return fail(c, SPSLAM_ERR_ARG, "spslam_place_min_score: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t K = (size_t)n_kf;
    const spslam_place_problem P{0, n_kf, query, 0};
    const DbStage ds(*db, n_kf, nullptr);
    enum { kOrdered = DbStage::kFirst, kNOrdered, kBad, kProblem, kOut };
    Stage st(c);
    if (int rc = ds.open(st, {{graph->ordered, K * (size_t)graph->stride * 4}, {graph->n_ordered, K * 4},
                              {kf_bad, kf_bad ? K : 0, K}, {&P, sizeof P}, sizeof(float)}))
        return rc;
    const spslam_place_db dd = ds.device(st, false);
    spslam_covis_graph dg{};
    dg.ordered = st.slot<int32_t>(kOrdered);
    dg.n_ordered = st.slot<int32_t>(kNOrdered);
    dg.stride = graph->stride;
    int rc = spslam_place_min_score_batch_device(c, 1, st.slot<spslam_place_problem>(kProblem), &dd, &dg,
                                                 kf_bad ? st.slot<uint8_t>(kBad) : nullptr, st.slot<float>(kOut),
                                                 c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(min_score, st.slot<void>(kOut), sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

}  // extern "C"
