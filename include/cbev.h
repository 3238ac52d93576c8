/*
 * cbev.h — C-ABI of the MI355X batched CarlaBEV step (libcbev.so).
 *
 * The reference has no FFI: its "operator API" for this path is the Gymnasium
 * surface of `CarlaBEV.envs.carlabev.CarlaBEV` wrapped by `make_env`
 * (`CarlaBEV/envs/__init__.py:108-120`, a `SyncVectorEnv`). Each entry point
 * below replaces the per-env Python call chain named next to it, batched over
 * N environments whose state lives in device memory as fixed-size records
 * (include/cbev_layout.h). The Python facade (carlabev_env_amd/vector_env.py)
 * binds these symbols with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions: every buffer argument is a plain device pointer (HBM) unless
 * named *_host; sizes are element counts; `stream` is a hipStream_t passed as
 * void* (NULL = default stream). All launches are asynchronous on `stream`.
 * Functions return 0 on success and a negative code on error; the message is
 * available from cbev_last_error() (thread-local). Calls on one context are
 * not re-entrant.
 */
#ifndef CBEV_H
#define CBEV_H

#include <stdint.h>

#include "cbev_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CBEV_ABI_VERSION 7

typedef struct cbev_ctx cbev_ctx;

/* error codes */
enum { CBEV_OK = 0, CBEV_EINVAL = -1, CBEV_EHIP = -2, CBEV_ESTATE = -3 };

int cbev_abi_version(void);
int cbev_params_size(void);                         /* sizeof(cbev_params) */
int cbev_layout_of(const cbev_caps* caps, cbev_layout* out);
/* comma-separated field names of a record group: 0 HD, 1 HI, 2 AD, 3 AI, 4 TI */
const char* cbev_field_names(int group);
const char* cbev_last_error(void);

/* Context = the static world of `CarlaBEV._setup` (carlabev.py:56-72):
 * renderer geometry, action table, reward parameters, record capacities.
 * Replaces `BaseMap.__init__` (world.py:33-67) + `build_reward_fn`. */
int cbev_create(const cbev_params* params, const cbev_caps* caps, int device, cbev_ctx** out);
void cbev_destroy(cbev_ctx* ctx);

/* Upload the padded class map (render surface of world.py:_build_padded_render_map,
 * one palette id per texel, render_h rows of map_pitch bytes). Host pointer,
 * copied into context-owned HBM. Replaces load_map (envs/utils.py:49-62). */
int cbev_set_map(cbev_ctx* ctx, const uint8_t* padded_map_host, int64_t bytes);

/* One `CarlaBEV.step(action)` (carlabev.py:223-231) for n envs: k_actors (when
 * the record has actor slots), k_ego (ego update + collision / reward /
 * termination), k_raster (the observation), in that order on `stream`:
 *   records      n state records (record_bytes each), updated in place
 *   actions      int32[n] discrete indices, or float32[n][3] continuous
 *   frames       uint8[n][S][S] palette-id observation (render(), carlabev.py:233-249)
 *   reward       float64[n]; term, trunc uint8[n]; cause int32[n] (CBEV_CAUSE_*)
 *   info         float32[n][CBEV_INFO_FLOATS] per-step comfort/control export or NULL */
#define CBEV_INFO_FLOATS 16
int cbev_step(cbev_ctx* ctx, void* records, int n, const void* actions, uint8_t* frames, double* reward,
              uint8_t* term, uint8_t* trunc, int32_t* cause, float* info, void* stream);

/* Action repeat (frame skip): `repeat` CarlaBEV.step calls with the same
 * actions and one observation, as a FrameSkip(repeat) wrapper directly around
 * each env would give. Substep 1 is cbev_step's (nothing freezes it). An env
 * whose substep j < repeat was terminal (term, truncation included) is frozen
 * for the rest of the call: its record is not touched, its actors do not move,
 * it writes no second episode row and counts no second termination.
 *   reward       r1 + .. + rj in float64, in that order (j: the env's last executed substep)
 *   term, trunc, cause, info   those of the env's last executed substep
 *   frames       one render at the end, of every record as it then stands
 * KSTEPS (max_actions), EP_LEN and the episode accumulators count substeps.
 * With episode statistics every substep's rows go into the same ring slot (the
 * slot advances once per call; an env terminates at most once per call).
 * repeat == 1 is cbev_step. repeat outside [1, CBEV_REPEAT_MAX] is CBEV_EINVAL
 * before anything is launched. A deferred reset is launched (as by cbev_flush)
 * rather than folded. All launches are one chain on `stream`; nothing is
 * allocated. cbev_reset_terminated after it resets the envs whose term is set.
 * With cbev_profile on, a call with repeat > 1 records: before substep 1,
 * after its k_actors, after the last substep's ego kernel, after k_raster. */
#define CBEV_REPEAT_MAX 64
int cbev_step_repeat(cbev_ctx* ctx, void* records, int n, const void* actions, int repeat, uint8_t* frames,
                     double* reward, uint8_t* term, uint8_t* trunc, int32_t* cause, float* info, void* stream);

/* The masked step: cbev_step_repeat for the envs whose byte of `active`
 * (uint8[n] on the device, read when the launches run) is not 0; the others
 * stand still.
 * An active env does what cbev_step_repeat(..., repeat, ...) does for it, bit
 * for bit: substep 1 is never frozen by `term`, substeps 2..repeat are frozen
 * from its terminal substep on.
 * An inactive env: its record (RS_*, vis / vis_draw and the actors included)
 * is untouched, its actors and lights do not move, it writes no episode row
 * and changes no termination count or Stats accumulator, its action is not
 * decoded (no error flag), reward[e] = 0.0, and term[e], trunc[e], cause[e]
 * and its info row are left as they were. Its S*S bytes of `frames` become
 * those of `prev_frames` (the caller's previous newest ring slot; both 16-byte
 * aligned); prev_frames == frames leaves them untouched. Nothing is rendered
 * for it.
 * The checks are cbev_step_repeat's, plus non-null `active` and `prev_frames`;
 * every refusal is CBEV_EINVAL before anything is launched. A deferred reset
 * is launched first. One chain on `stream`, nothing allocated, capturable. The
 * episode-statistics slot advances once per call; cbev_reset_terminated works
 * after it; cbev_profile records the four events of a repeat call. repeat == 1
 * runs the same (unsplit) chain: the call never forwards to cbev_step. */
int cbev_step_masked(cbev_ctx* ctx, void* records, int n, const void* actions, const uint8_t* active, int repeat,
                     const uint8_t* prev_frames, uint8_t* frames, double* reward, uint8_t* term, uint8_t* trunc,
                     int32_t* cause, float* info, void* stream);

/* The masked step with a frame-stack head per env: cbev_step_masked for
 * everything but the frames. `ring` is the whole frame ring,
 * uint8[n_frames][n][S][S] (16-byte aligned), and heads (uint8[n] on the
 * device) holds the ring slot of each env's newest frame.
 * An active env: heads[e] = (heads[e] + 1) % n_frames, once per call whatever
 * `repeat` is and whichever substep ends the env, and its frame is rendered
 * into ring[heads[e]][e]. The head is advanced in place on the device by the
 * first substep's ego kernel (one thread per env), an earlier launch of the
 * stream than the raster, whose tiles only read it: a captured call replays
 * correctly.
 * An inactive env: heads[e] and all its ring slots are untouched, nothing is
 * rendered or copied for it (there is no prev_frames), and the rest is
 * cbev_step_masked's contract: record, actors, statistics and counts
 * untouched, reward 0, term / trunc / cause / info kept, no error flag.
 * The kernels reduce heads[e] modulo n_frames before they form an address, so
 * a byte >= n_frames is a caller error with unspecified frame order for that
 * env, never an access outside `ring`.
 * cbev_reset, cbev_reset_masked, cbev_reset_terminated and cbev_reset_frames
 * write a reset env's frame into all n_frames slots, so any head value is
 * right after a reset: resets neither read nor write `heads`.
 * Refusals (CBEV_EINVAL before anything is launched, the context as it was):
 * cbev_step_masked's, null `ring` or `heads`, n_frames outside [1, 255], a
 * ring that is not 16-byte aligned. A deferred reset is launched first. One
 * chain on `stream`, nothing allocated, capturable; the episode-statistics
 * slot advances once; cbev_reset_terminated works after it; cbev_profile
 * records the four events of the masked call. */
int cbev_step_heads(cbev_ctx* ctx, void* records, int n, const void* actions, const uint8_t* active, int repeat,
                    uint8_t* ring, int n_frames, uint8_t* heads, double* reward, uint8_t* term, uint8_t* trunc,
                    int32_t* cause, float* info, void* stream);

/* Episode statistics on the device (Stats, src/deeprl/stats.py:87-148, and
 * CarlaBEV._check_termination, carlabev.py:177-185), so `infos["episode_info"]`
 * needs no per-step host work. The caller owns the buffers (device memory):
 *   stats   cbev_episode_stats[n], zeroed before first use, kept across episodes
 *   rows    float64[ring][n][CBEV_EP_COUNT]; counts int32[ring], zeroed
 * Step s (the s-th cbev_step after this call, from 0) writes one row per env
 * that terminated into rows[s % ring] (in no particular order, counts[s % ring]
 * of them) and zeroes counts[(s + 1) % ring], so a slot stays readable until
 * step s + ring - 1 is queued (ring >= 3). cbev_reset / cbev_reset_frames stamp
 * each reset env's episode start on the device clock (CBEV_EP_SECONDS).
 * stats = NULL turns it off. Not stream-ordered: call it between steps. A slot
 * holds at most n rows: a step replayed from a graph (which zeroes the same next
 * slot every replay) keeps counting in counts[] but writes no row past them. */
int cbev_set_episode_stats(cbev_ctx* ctx, void* stats, int n, double* rows, int32_t* counts, int ring);
/* Slot of the latest step's rows (-1 when off) and the step count. */
int cbev_episode_slot(const cbev_ctx* ctx, int64_t* step_count);
/* Rate of the device clock the episode times use. */
int cbev_wall_clock_hz(const cbev_ctx* ctx, double* hz);

/* Episodes terminated in all cbev_step calls since cbev_create (synchronises):
 * the reset demand a host scene feed has to meet. */
int cbev_termination_count(cbev_ctx* ctx, int64_t* count);

/* Errors the kernels detect are not stream-ordered return codes: they set bits
 * of a context error word, read (and cleared, if clear != 0) by this call,
 * which synchronises the device.
 *   CBEV_ERR_ACTION_INDEX  a discrete action outside [-n, n) (the reference's
 *                          IndexError in discrete_actions[int(action)],
 *                          envs/spaces.py:46); that env stepped action 0.
 *                          Negative indices in [-n, 0) count from the end. */
#define CBEV_ERR_ACTION_INDEX 1
/*   CBEV_ERR_RASTER_WINDOW a raster tile's crop window exceeded its LDS bound
 *                          (an internal invariant; the frame is not valid). */
#define CBEV_ERR_RASTER_WINDOW 2
/*   CBEV_ERR_RETREAT_ROUTE a StopReturn retreat would rebuild a route of more
 *                          than 64 points in a context of at most 64 actor
 *                          slots (scene packing refuses such actors; that actor
 *                          keeps its route) */
#define CBEV_ERR_RETREAT_ROUTE 4
int cbev_error_flags(cbev_ctx* ctx, int32_t* flags_host, int clear);

/* Reset the envs selected by mask (uint8[n], NULL = all):
 *   if bank != NULL: records[i] = bank[b] with b = bank_idx[i], or, when
 *   bank_idx == NULL, b = (i + bank_offset) % n_bank (device-side scene bank);
 *   then render the reset observation (BaseMap.reset: theta = 0, no actors,
 *   world.py:92-100) into every slot of frames = uint8[n_frames][n][S][S]
 *   (the frame-stack ring: FrameStackObservation pads with the reset frame;
 *   n_frames = 1 for a plain frame buffer).
 * Replaces `CarlaBEV.reset` after scene generation (carlabev.py:96-148) and the
 * wrappers' reset path. One launch. */
int cbev_reset(cbev_ctx* ctx, void* records, int n, const void* bank, int n_bank, const uint8_t* mask,
               const int32_t* bank_idx, int bank_offset, uint8_t* frames, int n_frames, void* stream);

/* Reset observations of a static scene bank, rendered once: frames = uint8[n_bank][S][S],
 * frames[b] = the observation cbev_reset would render for bank[b] (BaseMap.reset draws
 * no actors, world.py:92-100, so it depends on the bank record only).
 * The bank-edit rule: the bytes of a bank row that a context has been given (here
 * or in a cbev_reset_masked / cbev_reset_terminated call) may change only before
 * a cbev_bank_frames call on that context that renders the row again. The cached
 * frames need this anyway; the reset preview (cbev_set_reset_preview) relies on
 * it too: a row's inputs fetched when an env terminates are used by the next
 * step's reset unless this call came in between (it discards every fetched
 * row on `stream`, so a captured step replayed after it sees none either). */
int cbev_bank_frames(cbev_ctx* ctx, const void* bank, int n_bank, uint8_t* frames, void* stream);

/* cbev_reset from a bank whose reset observations were rendered by cbev_bank_frames:
 * the same records and ring contents as cbev_reset(ctx, records, n, bank, n_bank, mask,
 * bank_idx, bank_offset, frames, n_frames, stream), by copies only. */
int cbev_reset_frames(cbev_ctx* ctx, void* records, int n, const void* bank, int n_bank, const uint8_t* mask,
                      const int32_t* bank_idx, int bank_offset, const uint8_t* bank_frames, uint8_t* frames,
                      int n_frames, void* stream);

/* `reset(options={"reset_mask": mask})` (SyncVectorEnv.reset -> CarlaBEV.reset,
 * carlabev.py:96-148) from a bank with cached reset frames, each reset after a
 * termination a fresh bank row: every env with mask[e] != 0 (uint8[n], read
 * when the launch runs) takes bank row (e + j * cbev_bank_stride(n_bank)) %
 * n_bank, j = the env's terminations so far (counted by cbev_step on the device
 * from 0 at cbev_create; the stride is coprime with n_bank, so each env walks
 * the whole bank before a scene repeats for it; a reset with no termination
 * since the last one takes the same row again). The row of an env depends on
 * that env alone and no reset writes the counts (ABI 7; before, a global cursor
 * dealt rows in env-id order, which made every workgroup of the folded reset
 * read the whole mask). Records and ring contents as cbev_reset_frames with
 * those bank rows. One launch, no host sync; n <= 2^20. */
int cbev_reset_masked(cbev_ctx* ctx, void* records, int n, const uint8_t* mask, const void* bank, int n_bank,
                      const uint8_t* bank_frames, uint8_t* frames, int n_frames, void* stream);
/* The canonical loop's reset, `reset(options={"reset_mask": terminated})`
 * (tools/debug_env.py:56-132): cbev_reset_masked with mask = the `term` buffer
 * of the last cbev_step on this context (n must be that step's n). */
int cbev_reset_terminated(cbev_ctx* ctx, void* records, int n, const void* bank, int n_bank,
                          const uint8_t* bank_frames, uint8_t* frames, int n_frames, void* stream);
/* The terminal observations of a same-step autoreset: the frame stacks of the
 * envs `mask` selects, compacted in env order, to be called between the step
 * and the reset that overwrites all their ring slots.
 *   ring       uint8[n_frames][n][h][w], h x w = the cbev_set_obs_size size (the
 *              render size by default), as the expansion calls take it
 *   heads      uint8[n] on the device, the slot of each env's newest frame
 *              (reduced modulo n_frames before any address is formed; `head` is
 *              then ignored), or NULL: the global `head` in [0, n_frames)
 *   mask       uint8[n] on the device, read when the launch runs; any nonzero
 *              byte selects the env; any alignment
 * With e_0 < e_1 < ... < e_(k-1) the selected envs and H_e the head of env e:
 *   out        uint8[n_frames][n][h][w]: out[f][r] = ring[(H_(e_r) + 1 + f) % n_frames][e_r]
 *              for r < k, the stacks oldest first, so `out` is itself a
 *              global-head ring with head n_frames - 1 (cbev_expand_obs_typed with
 *              n = k of its first k rows per slot); rows r >= k are not written
 *   out_env    int32[n]: e_r for r < k, -1 for k <= r < n
 *   out_count  int32[1]: k
 * No atomics: every workgroup ranks the whole mask itself (as cbev_reset_masked's
 * kernel does), so the order is by env id, no workgroup depends on another, and
 * a captured call replays with the mask as it is at replay time. 16-byte
 * aligned ring and out with h * w % 16 == 0 take 16-byte copies, anything else
 * a byte copy. A deferred reset is launched first. One launch on `stream`,
 * nothing allocated, capturable. CBEV_EINVAL before anything is launched: a
 * null ctx, ring, mask, out, out_env or out_count; n_frames outside [1, 255];
 * heads == NULL with head outside [0, n_frames); n > 2^20; out's bytes
 * overlapping the ring's. n <= 0 returns CBEV_OK and does nothing. */
int cbev_final_frames(cbev_ctx* ctx, const uint8_t* ring, int n, int n_frames, int head, const uint8_t* heads,
                      const uint8_t* mask, uint8_t* out, int32_t* out_env, int32_t* out_count, void* stream);

/* The sum of the per-env termination counts (synchronises the device): the
 * bank rows the canonical loop's resets have handed out since cbev_create. */
int cbev_bank_cursor(cbev_ctx* ctx, int64_t* cursor);
/* The per-env termination counts j of envs 0 .. n-1 (synchronises). */
int cbev_reset_counts(cbev_ctx* ctx, uint32_t* counts_host, int n);
/* The stride of the masked reset's bank rows for a bank of n_bank rows (-1 if n_bank < 1). */
int cbev_bank_stride(int n_bank);
/* Deferred canonical reset (off by default). With it on, cbev_reset_terminated
 * records the reset instead of launching it, and the next cbev_step of the same
 * records and frame ring folds it into its first kernel (k_ego; the envs take
 * the same bank rows, records and ring slots end up as cbev_reset_masked leaves
 * them, the mask is read when that step runs): the canonical loop's
 * step -> reset(reset_mask=terminated) -> step costs no reset launch. Any other
 * call on the context that reads or writes its state (every cbev_reset* call,
 * cbev_expand_obs, cbev_vector_obs, cbev_resize_obs, cbev_pack_frames,
 * cbev_bank_cursor, cbev_profile_raster, ...) or a cbev_step that cannot take
 * it first launches it on the stream it was recorded on, as does cbev_flush.
 * A caller that reads the records, the frame ring or writes the term buffer
 * itself calls cbev_flush first. Only records without actor slots (k_ego is the
 * step's first kernel) fold; otherwise cbev_reset_terminated launches at once.
 * The deferral is host-side state, taken when cbev_step is called: a cbev_step
 * captured into a graph while a reset is pending carries the folded reset, so
 * every replay resets the envs its term buffer selects at replay time (the mask
 * and the termination counts are read on the device); cbev_flush before capturing a
 * step that must not reset. Neither call allocates (safe under a global-mode
 * stream capture). */
int cbev_set_deferred_reset(cbev_ctx* ctx, int on);
/* 1 when a deferred reset is recorded and not yet applied. */
int cbev_reset_pending(const cbev_ctx* ctx);
/* Launch a recorded deferred reset (k_reset_mask) now; no-op otherwise. */
int cbev_flush(cbev_ctx* ctx);

/* The split step: cbev_step launches the ego update's front alone (k_ego_head:
 * everything the observation needs) and its collision / reward / termination
 * tail as the leading workgroups of the raster's launch, beside the render
 * instead of before it. Results are bit-identical either way. On by default
 * where supported; on = 0 selects the unsplit k_ego. Not supported at size 64
 * or where no tail group fits the raster's LDS: on = 1 then returns
 * CBEV_EINVAL (cbev_last_error says why) and the unsplit step stays. Host-side
 * state, taken when cbev_step is called; does not allocate. */
int cbev_set_split_step(cbev_ctx* ctx, int on);

/* The reset preview of the split step's folded reset. When the tail of a step
 * that folded a reset terminates env e, it also fetches the seven inputs (X, Y,
 * YAW, V, ACC, TSPEED, T) of the bank row e's next reset will take into a
 * context-owned buffer (64 bytes per env, 2^20 entries = 64 MB, allocated by
 * cbev_create where the preview can be on, nowhere else); the next step's k_ego_head then computes the reset envs in the
 * same pass as the kept ones instead of in a second pass behind a dependent
 * miss. A preview is taken only if the immediately preceding step entry on the
 * context wrote it, that entry folded a reset from the same bank pointer and
 * n_bank, no cbev_bank_frames or cbev_reset_masked / flushed reset ran in
 * between, and its row is the one the head computes itself from the env's
 * count; every other reset env takes the two-pass path, so a replayed captured
 * step uses previews in its first replay only. Scheduling only: results are
 * bit-identical either way (see the bank-edit rule at cbev_bank_frames). On by
 * default where the split step is supported and the records have no actor
 * slots; on = 1 elsewhere returns CBEV_EINVAL. Host-side state, taken when
 * cbev_step is called; does not allocate. */
int cbev_set_reset_preview(cbev_ctx* ctx, int on);
/* out[0]: the reset envs k_ego_head computed from a preview (one pass), out[1]:
 * those it computed from the bank row (two passes), since cbev_create.
 * Launches a deferred reset and synchronises, like cbev_reset_counts. */
int cbev_reset_preview_counts(cbev_ctx* ctx, uint64_t out[2]);

/* Wrapper stack on the device (wrap_env, envs/__init__.py:62-83). `ring` holds
 * n_frames frames per env (uint8[n_frames][n][h][w], slot `head` the newest;
 * h x w = the cbev_set_obs_size size, the render size by default):
 *   kind 0: semantic one-hot (rgb_to_semantic.py:65-142) + FrameStack + Flatten
 *           -> float32[n][F*C][h][w]; channel_lut[id] = bitmask of channels set
 *   kind 3: semantic + FrameStack + VehicleTemporalFusionWrapper
 *           (rgb_to_semantic.py:152-166,275-301) -> float32[n][C+2][h][w]
 *   kind 4: semantic + FrameStack + WeightedVehicleHistoryWrapper
 *           (rgb_to_semantic.py:169-191,304-332) -> float32[n][C][h][w]
 *           (kinds 3/4: the vehicle channel is the bit channel_lut[CBEV_PX_VEHICLE]
 *           sets; n_frames >= 3)
 *   kind 1: grayscale (gymnasium GrayscaleObservation) + FrameStack
 *           -> uint8[n][F][h][w]; channel_lut[id] = gray value
 *   kind 5: FrameStack of a ring that already holds gray values (cbev_resize_obs
 *           with gray = 1) -> uint8[n][F][h][w]; channel_lut unused (may be NULL)
 *   kind 2: RGB (render(), no wrappers) -> uint8[n][S][S][3] of the newest
 *           render-size frame; channel_lut[id] = 0xRRGGBB
 * C = n_channels. */
int cbev_expand_obs(cbev_ctx* ctx, const uint8_t* ring, int n, int n_frames, int head, int kind, int n_channels,
                    const uint32_t* channel_lut_host, void* out, void* stream);

/* Wire types of the semantic kinds (0, 3, 4). Every value of a semantic
 * observation is 0 or 1 (kind 4's last channel: 0, 0.25, 0.5, 0.75 or 1), so
 * the compact ones are lossless; Cout is the channel count of the kind above:
 *   CBEV_OBS_F32   float32[n][Cout][h][w]: what cbev_expand_obs writes, by the
 *                  same kernel family and host path as the types below
 *   CBEV_OBS_F16   float16[n][Cout][h][w] (kind 4: summed and clipped in float32, then converted)
 *   CBEV_OBS_U8    uint8[n][Cout][h][w], 0 or 1; kinds 0 and 3
 *   CBEV_OBS_BITS  uint8[n][Cout][ceil(h*w / 8)]: pixel p of a channel plane is
 *                  bit p & 7 of byte p >> 3 (numpy.packbits(plane.reshape(-1),
 *                  bitorder="little")), the unused high bits of a plane's last
 *                  byte are 0; kinds 0 and 3
 * cbev_expand_obs_typed takes cbev_expand_obs's arguments and checks, and returns
 * CBEV_EINVAL before it launches anything for an unknown out_dtype, for kind 4
 * with U8 or BITS, and for kinds 1, 2, 5 (uint8 already: they forward to
 * cbev_expand_obs) with an out_dtype other than CBEV_OBS_U8. It allocates
 * nothing (safe under stream capture). 16-byte-aligned ring and out take the
 * wide kernels; any alignment of the element type is accepted.
 * cbev_unpack_obs is the learner's side of CBEV_OBS_BITS: packed =
 * uint8[rows][ceil(pixels / 8)] (any number of planes, e.g. a minibatch gathered
 * from a rollout buffer) -> out[rows][pixels] of CBEV_OBS_F32, F16 or U8. */
#define CBEV_OBS_F32 0
#define CBEV_OBS_F16 1
#define CBEV_OBS_U8 2
#define CBEV_OBS_BITS 3
int cbev_expand_obs_typed(cbev_ctx* ctx, const uint8_t* ring, int n, int n_frames, int head, int kind, int n_channels,
                          const uint32_t* channel_lut_host, int out_dtype, void* out, void* stream);
/* cbev_expand_obs_typed of a ring with a head per env (cbev_step_heads): heads
 * = uint8[n] on the device, heads[e] the slot of env e's newest frame, so its
 * frame f (oldest first) is slot (heads[e] + 1 + f) % n_frames. The stacked
 * kinds: 0, 3, 4 in the wire types above, 1 and 5 as CBEV_OBS_U8; kind 2 (the
 * newest frame alone) is refused, and n_frames is at most 255. The other
 * checks, the kernel choice, the channel order and the arithmetic are the
 * typed call's; the kernels reduce heads[e] modulo n_frames. It allocates
 * nothing (capturable) and uses the cbev_set_obs_size size. */
int cbev_expand_obs_heads(cbev_ctx* ctx, const uint8_t* ring, int n, int n_frames, const uint8_t* heads, int kind,
                          int n_channels, const uint32_t* channel_lut_host, int out_dtype, void* out, void* stream);
int cbev_unpack_obs(cbev_ctx* ctx, const uint8_t* packed, int rows, int pixels, int out_dtype, void* out, void* stream);

/* obs_mode "vector" (CarlaBEV.render, carlabev.py:237-244): out = float32[n][7],
 * [x, y, yaw, v] of the hero state + its Stanley set point [cx, cy, cyaw] at
 * target_idx (stanley_controller.py:140-148), from the records as they are now. */
int cbev_vector_obs(cbev_ctx* ctx, const void* records, int n, float* out, void* stream);

/* The multi-GPU frame gather's wire format (palette ids are
 * <= 15): packed = uint8[n][S*S/2], byte j of env e = frames[e][2j] |
 * frames[e][2j + 1] << 4. cbev_unpack_frames is the inverse. The reference has
 * no multi-process path (SyncVectorEnv, envs/__init__.py:116-119): this halves
 * the bytes the gather of the compact observation moves over xGMI. frames must be
 * 16-byte and packed 8-byte aligned (CBEV_EINVAL otherwise). */
int cbev_pack_frames(cbev_ctx* ctx, const uint8_t* frames, int n, uint8_t* packed, void* stream);
int cbev_unpack_frames(cbev_ctx* ctx, const uint8_t* packed, int n, uint8_t* frames, void* stream);

/* EnvConfig.fov_masked: FovRenderer's static corner mask (envs/fov.py:46-68,96-99)
 * applied by the raster (step and reset frames) after compose, before the ego
 * overlay. mask_host = uint8[S][S], 0xff where the output is blacked out, 0
 * elsewhere (carlabev_env_amd/fov_mask.py builds pygame's polygon fill); NULL
 * turns the mask off. Not stream-ordered: call it before queuing work. */
int cbev_set_fov_mask(cbev_ctx* ctx, const uint8_t* mask_host);

/* ResizeObservation(obs_size) (gymnasium; cv2.resize INTER_AREA) between the
 * render and the mask / grayscale wrappers (envs/__init__.py:62-67). Sets the
 * wrapped frame size h x w (<= size; h == w == size turns resizing off) and
 * builds the INTER_AREA tables. Not stream-ordered: call it before queuing work. */
int cbev_set_obs_size(cbev_ctx* ctx, int h, int w);

/* Resize n palette-id frames (uint8[n][S][S], e.g. cbev_step's output) to the
 * cbev_set_obs_size size, fused with the next wrapper's colour test:
 *   gray = 0: out byte = the palette id whose colour equals the resized RGB,
 *             else CBEV_PX_OFF_PALETTE (all semantic channels 0) -> expand kinds 0/3/4
 *   gray = 1: out byte = the grayscale value of the resized RGB -> expand kind 5
 * Envs with mask[e] == 0 are skipped (mask NULL = all). The frame is written to
 * n_out destinations out + k*out_stride (e.g. every slot of the ring on reset).
 * Returns CBEV_ESTATE when no resize is configured. */
int cbev_resize_obs(cbev_ctx* ctx, const uint8_t* frames, int n, const uint8_t* mask, int gray, uint8_t* out,
                    int n_out, int64_t out_stride, void* stream);

/* Kernel timing with HIP events recorded on the step's own stream around each
 * step kernel (used by bench.py for the roofline figure). cbev_profile(ctx, 1)
 * resets the counters and starts recording (up to 8192 steps);
 * cbev_profile_read synchronises on the last event and returns the summed
 * milliseconds of [k_actors, k_ego, k_raster] and the step count (the split
 * step: the second span is k_ego_head, the third k_raster's launch with the ego
 * tail in it; cbev_profile_raster below always times the raster alone). */
int cbev_profile(cbev_ctx* ctx, int enable);
int cbev_profile_read(cbev_ctx* ctx, double* ms3, int64_t* steps);

/* Average duration of one k_raster launch over `reps` back-to-back launches on
 * `stream`, timed with two HIP events around the burst (bench.py's roofline
 * figure: the per-kernel events of cbev_profile also count each launch's
 * dispatch gap). It re-renders the observation of the current records, so
 * call it right after a cbev_step (which writes the render set-up and the
 * drawn target bits) and before any reset: `frames` then receives the bytes
 * that step wrote. Synchronises; writes the milliseconds per launch to *ms. */
int cbev_profile_raster(cbev_ctx* ctx, void* records, int n, uint8_t* frames, int reps, void* stream, double* ms);

#ifdef __cplusplus
}
#endif

#endif /* CBEV_H */
