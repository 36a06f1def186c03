/*
 * mbrwt.h -- C ABI of the MI355X-native Multi-BRWT row-query engine
 * (genome_graph_annotation_amd/libmbrwt.so).
 *
 * Drop-in boundary for the reference's BRWT query path
 * (ratschlab/genome_graph_annotation; paths below are relative to its root):
 *
 *   reference                                        replaced by
 *   -----------------------------------------------  -----------------------------------
 *   BinaryMatrix::get_row        common/binary_matrix.hpp:21      mbrwt_get_rows / _device (batched)
 *   BRWT::get_row                annotation/hierarchical_annotation/BRWT.cpp:26-53
 *   BRWT::get                    BRWT.cpp:9-24                     mbrwt_get_batch / _device
 *   BRWT::get_column             BRWT.cpp:55-85 (select1,          mbrwt_get_column / _device
 *                                bit_vector.cpp:863-869)
 *   bit_vector_rrr<63>::rank1    common/bit_vector.cpp:857-861     (inside the traversal kernel)
 *   bit_vector_rrr<63>::operator[]  common/bit_vector.cpp:884-888  (inside the traversal kernel)
 *   utils::RangePartition::get   common/utils.cpp:689-691          (leaf column table, composed)
 *   BRWT::num_rows/num_columns   BRWT.hpp:33-34                    mbrwt_num_rows / mbrwt_num_columns
 *   BRWT::num_relations          BRWT.cpp:130-140                  mbrwt_num_relations
 *   BRWT::load (structure ingestion) BRWT.cpp:87-111               mbrwt_create (from a tree description)
 *   StaticBinRelAnnotator::count_labels annotation/annotate_static.cpp:149-162
 *                                                                  mbrwt_count_labels_device
 *
 * Conventions: plain pointers and sizes only; no C++ or torch types.  Every
 * function returns an MBRWT_* status code; nothing throws across the ABI.
 * Rows are uint64 (binary_matrix.hpp:11) and must be < mbrwt_num_rows().
 * Columns are emitted as uint32 (the reference stores them as uint32,
 * utils.hpp:442-444).  Output order per row is the reference's order: the
 * pre-order (DFS) of the BRWT's leaves (BRWT.cpp:45-51).
 *
 * Threading: a context may be used from several host threads; calls on one
 * context are serialised internally (the reference's get_row is const and
 * called concurrently from a ThreadPool, main.cpp:462-497).  Device-buffer
 * calls (*_device) may return with work still queued on the caller's stream;
 * the context orders its internal workspaces across streams (each call's
 * stream waits for the previous call's queued work, whichever stream that was
 * on), so calls on different streams are safe.  The caller's own output
 * buffers are ready when the caller's stream reaches them.
 */
#ifndef MBRWT_H
#define MBRWT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define MBRWT_OK 0
#define MBRWT_ERR_INVALID 1     /* bad argument or malformed tree description */
#define MBRWT_ERR_RANGE 2       /* row or column out of range (reference: assert, BRWT.cpp:27) */
#define MBRWT_ERR_CAPACITY 3    /* cols_cap too small; *cols_needed holds the size needed */
#define MBRWT_ERR_UNSUPPORTED 4 /* tree beyond this build's limits */
#define MBRWT_ERR_DEVICE 5      /* HIP runtime error (see mbrwt_last_error_message) */
#define MBRWT_ERR_NOMEM 6       /* device or host allocation failed */

typedef struct mbrwt_ctx mbrwt_ctx;

/* ---- structure ingestion ---------------------------------------------- */
/*
 * A BRWT in breadth-first numbering: node 0 is the root; the children of node
 * u are nodes [first_child[u], first_child[u] + num_children[u]) in the
 * reference's child order (BRWT.hpp:60).  vec_words[u] points to node u's
 * index column (BRWT.hpp:59 nonzero_rows_) as ceil(vec_size[u]/64) LSB-first
 * uint64 words.  For a leaf, leaf_column[u] is the global column id obtained by
 * composing RangePartition::get along the path (utils.cpp:689-691); internal
 * nodes carry UINT32_MAX.  num_nodes == 0 describes the empty BRWT().
 * Replaces BRWT::load (BRWT.cpp:87-111) as the way structure enters the engine.
 */
typedef struct mbrwt_tree_desc {
    uint64_t num_rows;
    uint64_t num_columns;
    uint32_t num_nodes;
    const uint32_t *num_children;
    const uint32_t *first_child;
    const uint32_t *leaf_column;
    const uint64_t *vec_size;
    const uint64_t *const *vec_words;
} mbrwt_tree_desc;

/* Build the device image of a BRWT on HIP device `device`. */
int mbrwt_create(const mbrwt_tree_desc *desc, int device, mbrwt_ctx **out);

/*
 * Generate a synthetic Multi-BRWT directly in device memory: the law of a
 * basic-partitioner (BRWT_builders.cpp:20-31) BRWT built from i.i.d.
 * Bernoulli(density) columns (experiments/data_generation.cpp:20-29), drawn
 * top-down from a counter-based hash (spec: DESIGN.md "Synthetic matrices").
 * arity in [2, 12]; num_rows >= 2^32 builds row shards (mbrwt_num_shards).
 */
typedef struct mbrwt_synth_desc {
    uint64_t num_rows;
    uint64_t num_columns;
    double density;
    uint32_t arity;
    uint64_t seed;
} mbrwt_synth_desc;
int mbrwt_create_synthetic(const mbrwt_synth_desc *desc, int device, mbrwt_ctx **out);

/*
 * The same law over ANY tree shape (e.g. the shape of a greedy + relaxed tree,
 * the reference's production build path: transform_anno --greedy then
 * relax_brwt): BFS arrays as in mbrwt_tree_desc (children contiguous,
 * leaf_column = the leaf's global column, UINT32_MAX for internal nodes),
 * node arity <= 12; desc->arity is ignored and desc->num_columns must equal
 * the number of leaves.  q(u) = 1 - (1-density)^(leaves below u); node keys
 * are BFS ids.
 */
typedef struct mbrwt_shape_desc {
    uint32_t num_nodes;
    const uint32_t *num_children;
    const uint32_t *first_child;
    const uint32_t *leaf_column;
} mbrwt_shape_desc;
int mbrwt_create_synthetic_shaped(const mbrwt_synth_desc *desc, const mbrwt_shape_desc *shape, int device,
                                  mbrwt_ctx **out);

/*
 * Build a BRWT from its columns on the device: BRWTBottomUpBuilder::build
 * (BRWT_builders.cpp:119-163) with the basic partitioner of the given arity
 * (get_basic_partitioner, BRWT_builders.cpp:20-31; groups of one pass
 * through).  compute_or and generate_subindex run as HIP kernels; the result
 * is the image mbrwt_create would build from the same tree.  columns[j] is
 * column j over the rows as ceil(num_rows/64) LSB-first uint64 words in host
 * memory (bits past num_rows are ignored).  arity in [2, 64]; num_columns == 0
 * gives the empty BRWT().
 */
typedef struct mbrwt_columns_desc {
    uint64_t num_rows;
    uint64_t num_columns;
    const uint64_t *const *columns;
    uint32_t arity;
} mbrwt_columns_desc;
int mbrwt_create_from_columns(const mbrwt_columns_desc *desc, int device, mbrwt_ctx **out);

/*
 * BRWTOptimizer::relax(brwt, max_arity) (BRWT_builders.cpp:166-297;
 * `annograph relax_brwt --relax-arity`, main.cpp:746, config.cpp:104):
 * internal nodes whose removal saves space (pruning_delta, :351-380, with the
 * RRR size model of :315-321) are removed and their children re-attached to
 * the parent, within max_arity children per node.  The re-attached children's
 * index columns are expanded on the device.  Query results are unchanged.
 * mbrwt_create_from_columns_relaxed = mbrwt_create_from_columns then relax
 * (the reference's convert + relax_brwt); mbrwt_create_relaxed relaxes an
 * exported tree.  max_arity <= 1 leaves the tree as built.
 */
int mbrwt_create_from_columns_relaxed(const mbrwt_columns_desc *desc, uint64_t relax_max_arity, int device,
                                      mbrwt_ctx **out);
int mbrwt_create_relaxed(const mbrwt_tree_desc *desc, uint64_t max_arity, int device, mbrwt_ctx **out);

/*
 * Build the row records straight from row-major data: the
 * rows as a CSR (as mbrwt_binrel_desc, mbrwt_wt.h) plus a tree SHAPE.  A row's
 * record is a function of its label set and the shape alone, and the BRWT
 * over a given shape is unique, so the context answers every query -- and
 * mbrwt_tree_export gives every index column -- exactly as the ROWS context
 * mbrwt_create builds from that tree; but no node image and no dense column
 * ever exists: the device holds the records plus one range's labels (ranges
 * of multiples of 360,360 rows; the first, at most 64 x 360,360 rows, decides
 * the record code and layout; later ones are sized from the free device
 * memory less an 8 GiB reserve, at most 2^31 - 1 labels each;
 * MBRWT_BUILD_ROWS_RANGE fixes the size).  This is how a matrix too large for
 * mbrwt_create_from_columns (num_columns x ceil(num_rows / 64) words on the
 * host and the device) is built from data: the shape from the same rows
 * (mbrwt_tree_shape_from_rows: the greedy partitioner over its 10^6-row
 * sample, relax over all rows), the records from all rows, a .brwt through
 * mbrwt_tree_export + mbrwt_tree_serialize.  The reference's annotators
 * produce such rows (annotate_row, RowCompressed).
 *
 * shape == NULL: the basic partitioner's tree of `arity` (2..64) over
 * num_columns (mbrwt_tree_basic_shape); else the given shape (arity ignored):
 * BFS arrays as documented for mbrwt_shape_desc, node arity up to 64, whose
 * leaves' leaf_column must be a permutation of 0..num_columns-1
 * (MBRWT_ERR_INVALID otherwise, also when the leaf count differs).
 * Layout: always MBRWT_LAYOUT_ROWS.  The thread's MBRWT_BUILD_LAYOUT must be
 * AUTO or ROWS (NODES, BOTH: MBRWT_ERR_UNSUPPORTED -- there is no node image
 * to build); AUTO's decline of records above 1.25 requests per row does not
 * apply (there is nothing to fall back to).  Every other record option of the
 * calling thread is honoured as in a ROWS build from a tree
 * (MBRWT_BUILD_ROWS_CODE, _BLOCK, _VAR, _VAR_LANES, _CLASSES, _FOOTPRINT,
 * _RANGE, _ROWS_WGS_PER_CU).  A tree outside the row-record limits (a
 * one-column tree, arity > 64, columns beyond the records' u16 labels,
 * height > 16, a walk table over 8,192 words, a row of more than 32,767
 * labels in any range) ->
 * MBRWT_ERR_UNSUPPORTED with the messages of layout ROWS.
 * Rows are sets, their columns in any order: a column id >= num_columns or a
 * column listed twice in a row -> MBRWT_ERR_INVALID (both checked on the
 * device, as mbrwt_wt_create); offsets[0] != 0, descending offsets or null
 * arrays -> MBRWT_ERR_INVALID, checked on the host before any device call.
 * A null desc or out -> MBRWT_ERR_INVALID, with or without a GPU.
 * num_rows == 0 or num_columns == 0: the context mbrwt_create_from_columns
 * gives for the same empty matrix.  mbrwt_num_relations = the total number of
 * labels; mbrwt_num_nodes comes from the shape.
 */
typedef struct mbrwt_rows_desc {
    uint64_t num_rows, num_columns;
    const uint64_t *offsets; /* num_rows + 1, offsets[0] = 0, ascending */
    const uint32_t *cols;    /* row r: cols[offsets[r] .. offsets[r+1]), any order */
} mbrwt_rows_desc;
int mbrwt_create_from_rows(const mbrwt_rows_desc *desc, const mbrwt_shape_desc *shape, uint32_t arity, int device,
                           mbrwt_ctx **out);

/*
 * The same build from SPARSE COLUMNS: per column the
 * strictly ascending ids of its set rows -- the form the reference holds its
 * data in before a BRWT conversion (ColumnCompressed::data(), one bit vector
 * per label; bit_vector::call_ones gives a column's ids in this order).  The
 * rows are transposed on the device, range of rows by range of rows: every
 * column's slice of ids in the range is staged (u32, relative to the range's
 * first row), composed with the column's pre-order index, sorted stably by
 * row and handed to the record builders of mbrwt_create_from_rows.  The
 * context is the one mbrwt_create_from_rows gives on the same matrix: the
 * same image bytes, mbrwt_rows_stats, mbrwt_tree_export and answers.
 *
 * Shape, arity, layout (always ROWS; NODES, BOTH: MBRWT_ERR_UNSUPPORTED),
 * the record options of the calling thread, the limits and the empty
 * matrices are those of mbrwt_create_from_rows.  Ranges are multiples of
 * 360,360 rows sized like its ranges from the free device memory (here 24
 * bytes per label and 4 per row), at most 2^31 - 1 labels each;
 * MBRWT_BUILD_ROWS_RANGE fixes the size.
 * rows: u64 ids; rows32: the same as u32 (num_rows <= 2^32); exactly one of
 * the two is non-null (both null only without any label).
 * MBRWT_ERR_INVALID: a row id >= num_rows, ids of a column that do not ascend
 * strictly (unsorted, or a row twice) -- both found on the device, in the
 * range that holds them --; offsets[0] != 0, descending offsets, a null
 * offsets array, both rows and rows32, neither with labels present, rows32
 * with num_rows > 2^32 -- on the host before any device call; a null desc or
 * out, with or without a GPU.  A row of more than 32,767 labels:
 * MBRWT_ERR_UNSUPPORTED (seen on the device, from the range's row lengths).
 * A failed build frees everything it allocated.
 */
typedef struct mbrwt_sparse_columns_desc {
    uint64_t num_rows, num_columns;
    const uint64_t *offsets; /* num_columns + 1, offsets[0] = 0, ascending */
    const uint64_t *rows;    /* column c: rows[offsets[c] .. offsets[c+1]), strictly ascending; or NULL */
    const uint32_t *rows32;  /* the same as u32 (num_rows <= 2^32); exactly one of rows / rows32 non-null */
} mbrwt_sparse_columns_desc;
int mbrwt_create_from_sparse_columns(const mbrwt_sparse_columns_desc *desc, const mbrwt_shape_desc *shape,
                                     uint32_t arity, int device, mbrwt_ctx **out);

void mbrwt_destroy(mbrwt_ctx *ctx);

/* A second query context over the SAME device image (no copy): its own
 * workspaces, status block, events and host-buffer stream, so queries on a
 * context and on its clones may run concurrently on different streams (or
 * host threads) -- the reference's server answers concurrent requests from
 * one annotator (cli/server.cpp); calls on ONE context are ordered on its
 * workspace fence.  Options start at their defaults.  Destroying the source
 * while clones are alive defers the image's release to the last clone.
 * Sharded contexts clone their shards.  Replaces nothing in the reference:
 * its annotator is shared by reference across its worker threads. */
int mbrwt_ctx_clone(mbrwt_ctx *src, mbrwt_ctx **out);

/* ---- device layout ------------------------------------------------------
 * Two layouts of the same tree:
 *   NODES  per-node, sibling-interleaved index columns with ranks; get_row is
 *          the reference's rank1 descent (BRWT.cpp:26-53) over them;
 *   ROWS   ROW RECORDS: the tree's index bits regrouped by row (each row's
 *          descent -- the children mask of every internal node it reaches, in
 *          DFS pre-order -- stored with the row), so get_row is one block read
 *          and a record walk; the rank1 remaps are resolved at build time.
 *          Trees with arity <= 64 (r06; 16 before: nodes wider than 16
 *          need a tree of at most 8 internal levels), < 2^16 columns (2^15
 *          before), height <= 16, at most 32,767 labels in any one row (a
 *          row's count travels in 15 bits between the traversal and the
 *          CSR; the variable-length records have the same bound).  Built one
 *          range of rows at a time, so rows >= 2^32 need no row shards.
 *          get_column scans the records; mbrwt_tree_export rebuilds every
 *          index column from the records (so BinaryMatrix::serialize works).
 *   BOTH   both images: get_rows / count_labels on the records, the rest on
 *          the node image.
 * The layout is chosen when a context is created: mbrwt_set_build_option
 * (MBRWT_BUILD_LAYOUT, value) sets it for the mbrwt_create* / mbrwt_load calls
 * of the calling thread; MBRWT_LAYOUT_AUTO (the default) chooses: ROWS when
 * the tree is within the row-record limits, its records cost at most ~1.25
 * block requests per row (no dense-row shapes) and the image fits the
 * device, NODES otherwise.  Layout ROWS on a tree outside its limits ->
 * MBRWT_ERR_UNSUPPORTED.  No reference counterpart (the reference's BRWT has
 * one sdsl layout).
 */
#define MBRWT_BUILD_LAYOUT 1
/* (MBRWT_BUILD_PARTITIONER, value): the partitioner of the calling thread's
   mbrwt_create_from_columns[_relaxed] -- MBRWT_PARTITIONER_BASIC (default:
   groups of desc->arity consecutive nodes) or MBRWT_PARTITIONER_GREEDY
   (binary_grouping_greedy, partitionings.cpp:148-196, the `--greedy` build of
   scripts/kingsford/convert.sh:24; desc->arity is ignored): per level the
   inner products of every column pair over the reference's row sample
   (min(10^6, rows) rows, mt19937 seed 1) on the device, the candidate sort
   and the matching on the host as the reference does them. */
#define MBRWT_BUILD_PARTITIONER 2
#define MBRWT_PARTITIONER_BASIC 0
#define MBRWT_PARTITIONER_GREEDY 1
/* (MBRWT_BUILD_ROWS_FOOTPRINT, value): how the calling thread's row-record
   builds pick the block size and rows per block -- MBRWT_ROWS_FAST (default:
   the fewest modelled requests per row, then the smallest image within 2 %)
   or MBRWT_ROWS_COMPACT (the smallest image within 30 % of the fewest
   modelled requests: the greedy + relax shape at 3.7 B rows takes 158.90 GB
   instead of 236.85 GB for a 2 % slower kernel). */
#define MBRWT_BUILD_ROWS_FOOTPRINT 3
#define MBRWT_ROWS_FAST 0
#define MBRWT_ROWS_COMPACT 1
#define MBRWT_LAYOUT_AUTO 0
#define MBRWT_LAYOUT_NODES 1
#define MBRWT_LAYOUT_ROWS 2
#define MBRWT_LAYOUT_BOTH 3
/* Tuning and test options of the calling thread's builds (r05: these were
   environment variables read by the library; they are now explicit, scoped
   like the options above).  Every default is the automatic choice.
   MBRWT_BUILD_ROWS_VAR       -1 auto, 0 never, 1 always the variable-length
                              records of dense rows (uniform trees)
   MBRWT_BUILD_VAR_LANES      lanes per row of their decode (0 auto; 1..16, a
                              power of two)
   MBRWT_BUILD_ROWS_BLOCK     row-record blocks: 0 auto, else B << 8 | S (B 64 or
                              128 bytes, S rows per block)
   MBRWT_BUILD_ROWS_RANGE     rows per range of a ranged row-record build (0
                              auto; a multiple of 360,360)
   MBRWT_BUILD_NODE_KINDS     node-image kinds built (bit mask, default all):
                              MBRWT_KIND_FOLD_ROOT | _PACK | _PACK2 | _PACKT;
                              PACK2 / PACKT also need PACK
   MBRWT_BUILD_SHARD_ROWS     rows per row shard (0: 2^31; small values force
                              shards on small trees -- a test hook)
   MBRWT_BUILD_ROWS_WGS_PER_CU  resident workgroups per CU of the row-record
                              traversal (0 auto; occupancy sweeps)
   MBRWT_BUILD_ROWS_CLASSES   RECORD CLASSES of the block layout:
                              one copy of every distinct row record plus a
                              class index of ceil(log2 classes) bits per row,
                              for data whose rows repeat few label sets.
                              -1 auto (default: built when a tenth of a
                              2^20-row sample repeats a record, kept when
                              there are at most half as many classes as rows
                              and they at least halve the image), 0 never,
                              1 whenever they fit (always exact: every row's
                              record is compared with its class's)
   MBRWT_BUILD_ROWS_CODE      how a row record stores the row's descent
                              (DESIGN §4g, §4h): 0 (default) AUTO -- TERMINAL
                              RECORDS where they are smaller than byte masks,
                              else byte masks; 1 NIBBLE CODES -- a mask with
                              one bit set as that bit's index in 4 bits, any
                              other as 12 bits -- for uniform trees of arity
                              <= 8 (other trees keep bytes); 2 terminal
                              records where they fit: the leaf parents and
                              leaves the descent reaches, in pre-order, each
                              a field {id, its children mask} (masks <= 16
                              bits, <= 4,096 terminals); 3 one byte per 8
                              children of every internal node reached */
#define MBRWT_BUILD_ROWS_VAR 4
#define MBRWT_BUILD_VAR_LANES 5
#define MBRWT_BUILD_ROWS_BLOCK 6
#define MBRWT_BUILD_ROWS_RANGE 7
#define MBRWT_BUILD_NODE_KINDS 8
#define MBRWT_BUILD_SHARD_ROWS 9
#define MBRWT_BUILD_ROWS_WGS_PER_CU 10
#define MBRWT_BUILD_ROWS_CLASSES 11
#define MBRWT_BUILD_ROWS_CODE 12
#define MBRWT_KIND_FOLD_ROOT 1
#define MBRWT_KIND_PACK 2
#define MBRWT_KIND_PACK2 4
#define MBRWT_KIND_PACKT 8
#define MBRWT_KIND_ALL 15
int mbrwt_set_build_option(int option, int64_t value);
/* The calling thread's current value of a build option (so that a caller can
   restore it after a scoped change). */
int mbrwt_get_build_option(int option, int64_t *value);
int mbrwt_layout(const mbrwt_ctx *ctx); /* MBRWT_LAYOUT_NODES / _ROWS / _BOTH of a context */
/* Row-record image: out[0] block bytes B (0: the variable-length records of
   dense rows -- then [1] = 13 rows per directory line, [2] directory bytes),
   [1] rows per block S, [2] block
   bytes, [3] spill bytes, [4] record bytes (counts + masks), [5] spilled rows,
   [6] rows longer than a block, [7] tree height | K << 32, K = the internal
   levels above the leaf parents when every path has that many (the
   odometer walk of csrc/rows.hip), else 0.  MBRWT_ERR_UNSUPPORTED without
   row records. */
int mbrwt_rows_stats(const mbrwt_ctx *ctx, uint64_t out[8]);
/* Record classes of a row-record image: out[0] classes (0: none -- then the
   blocks hold one record per row), [1] class index bits per row, [2] class
   index bytes, [3] distinct records in the layout-AUTO sample (0: not
   sampled).  With classes, mbrwt_rows_stats describes the dictionary (one
   record per class, S = 1).  MBRWT_ERR_UNSUPPORTED without row records. */
int mbrwt_rows_classes(const mbrwt_ctx *ctx, uint64_t out[4]);
/* Diagnostics: what was built for one node of the per-node images (read-only;
   launches nothing).  dnode 0 is the super-root, dnode u + 1 is node u of the
   tree description (BFS numbering); `shard` picks the row shard of a sharded
   context (0 .. mbrwt_num_shards - 1) and must be 0 otherwise.  out[0] kind
   (MBRWT_NODE_*), [1] arity, [2] stride -- bytes per 32-position block of a
   PLANE node, 64 for a PACK node, positions per 64-byte block (1..8) for a
   PACK2 / PACKT node, 0 otherwise --, [3] length: the positions of the node's
   image, i.e. the rows that reach the node (0 for a leaf and for a folded
   root).  MASK8..MASK64: every child is a leaf, one mask of 1 / 2 / 4 / 8
   bytes per position.  FOLDED: the root whose children the super-root holds
   over the row positions.  A node that is MBRWT_NODE_PACKT_IN, or a
   PACK / MASK8 node below a PACK2 or PACK node, has a record but no image of
   its own.  MBRWT_ERR_RANGE for a dnode or shard that does not exist,
   MBRWT_ERR_UNSUPPORTED on a context that dropped its node images
   (MBRWT_LAYOUT_ROWS). */
#define MBRWT_NODE_LEAF 0
#define MBRWT_NODE_PLANE 1
#define MBRWT_NODE_MASK8 2
#define MBRWT_NODE_MASK16 3
#define MBRWT_NODE_MASK32 4
#define MBRWT_NODE_MASK64 5
#define MBRWT_NODE_FOLDED 6
#define MBRWT_NODE_PACK 7
#define MBRWT_NODE_PACK2 8
#define MBRWT_NODE_PACKT 9
#define MBRWT_NODE_PACKT_IN 10
int mbrwt_node_info(const mbrwt_ctx *ctx, uint64_t shard, uint32_t dnode, uint64_t out[4]);

/* ---- multi-device (one process, N GPUs) --------------------------------
 * A replica of the tree on every device of `devices` (n entries; a device
 * may repeat), built concurrently with the calling thread's build layout,
 * and get_rows over a batch cut into n contiguous slices -- slice r on
 * replica r -- reassembled into the caller's ONE CSR: host buffers
 * (mbrwt_multi_get_rows: device-to-host copies at each slice's label offset)
 * or device buffers on devices[0] (mbrwt_multi_get_rows_device: peer copies
 * over xGMI, `stream` on devices[0]).  Results, order and the capacity
 * protocol are those of mbrwt_get_rows over the whole batch.  The
 * reference's `annograph classify` runs its ThreadPool in one process
 * (main.cpp:462-497): this is how its host drives every GPU of a node.
 * mbrwt_multi_replica gives replica i's context (point / column queries,
 * properties, export); it is owned by the multi handle.
 *
 * What classify itself calls -- get_labels(indices, presence_ratio)
 * (main.cpp:193) and get_top_labels(indices, num_top) (main.cpp:177) -- runs
 * on every replica end to end: mbrwt_multi_get_labels_batch[_device] and
 * mbrwt_multi_get_top_labels_batch[_device] take the arguments of
 * mbrwt_get_labels_batch[_device] / mbrwt_get_top_labels_batch[_device]
 * (below) and return their output, order, tie order, errors and capacity
 * protocol over the whole batch (*labels_needed = the total of all
 * replicas).  The batch is cut between reads, not rows: replica r classifies
 * the whole reads [b_r, b_{r+1}), b_0 = 0, b_k = n_reads, and for 0 < r < k
 *     b_r = the first read whose first row offset is >= ceil(r * n_rows / k),
 * so no replica holds more than n_rows / k rows plus the longest read; a
 * replica may get no read; reads without rows at the front of the batch stay
 * on replica 0, those at the back on replica k - 1.  The read offsets are
 * validated as a whole (first 0, ascending, last n_rows) before any replica
 * runs: MBRWT_ERR_INVALID.  Only the rows (in) and each read's labels (out)
 * cross devices.  Device forms: inputs and outputs on devices[0], ordered on
 * `stream`; the outputs are complete on return.  When several replicas fail,
 * the status and message are those of the lowest one.  Calls on one handle
 * are serialised.
 */
typedef struct mbrwt_multi mbrwt_multi;
int mbrwt_multi_create(const mbrwt_tree_desc *desc, const int *devices, int n, mbrwt_multi **out);
int mbrwt_multi_create_synthetic(const mbrwt_synth_desc *desc, const int *devices, int n, mbrwt_multi **out);
int mbrwt_multi_load(const uint8_t *bytes, uint64_t len, uint64_t *consumed, const int *devices, int n,
                     mbrwt_multi **out);
void mbrwt_multi_destroy(mbrwt_multi *m);
int mbrwt_multi_size(const mbrwt_multi *m);
mbrwt_ctx *mbrwt_multi_replica(mbrwt_multi *m, int i);
int mbrwt_multi_get_rows(mbrwt_multi *m, const uint64_t *rows, uint64_t n, uint64_t *offsets, uint32_t *cols,
                         uint64_t cols_cap, uint64_t *cols_needed);
int mbrwt_multi_get_rows_device(mbrwt_multi *m, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets,
                                uint32_t *d_cols, uint64_t cols_cap, uint64_t *cols_needed, void *stream);
int mbrwt_multi_get_labels_batch(mbrwt_multi *m, const uint64_t *rows, uint64_t n_rows, const uint64_t *read_offsets,
                                 uint64_t n_reads, double presence_ratio, uint64_t *label_offsets, uint32_t *labels,
                                 uint64_t labels_cap, uint64_t *labels_needed);
int mbrwt_multi_get_labels_batch_device(mbrwt_multi *m, const uint64_t *d_rows, uint64_t n_rows,
                                        const uint64_t *d_read_offsets, uint64_t n_reads, double presence_ratio,
                                        uint64_t *d_label_offsets, uint32_t *d_labels, uint64_t labels_cap,
                                        uint64_t *labels_needed, void *stream);
int mbrwt_multi_get_top_labels_batch(mbrwt_multi *m, const uint64_t *rows, uint64_t n_rows,
                                     const uint64_t *read_offsets, uint64_t n_reads, uint64_t num_top,
                                     uint64_t *label_offsets, uint32_t *labels, uint64_t *counts, uint64_t labels_cap,
                                     uint64_t *labels_needed);
int mbrwt_multi_get_top_labels_batch_device(mbrwt_multi *m, const uint64_t *d_rows, uint64_t n_rows,
                                            const uint64_t *d_read_offsets, uint64_t n_reads, uint64_t num_top,
                                            uint64_t *d_label_offsets, uint32_t *d_labels, uint64_t *d_counts,
                                            uint64_t labels_cap, uint64_t *labels_needed, void *stream);

/* ---- files: the reference's BRWT stream (the matrix of a .brwt.annodbg) ----
 * An owned tree description (host memory).  Byte formats of sdsl-lite /
 * libmaus2 are restated from their published algorithms: PARITY UNPINNED
 * (no sdsl source or reference-written file exists here).
 *
 * mbrwt_tree_parse      BRWT::load (BRWT.cpp:87-111): the pre-order stream of
 *                       {RangePartition (utils.cpp:702-715), rrr_vector<63>
 *                       index (bit_vector.cpp:906-925), child count, children}
 *                       starting at bytes[0]; *consumed (may be NULL) = bytes
 *                       read.  MBRWT_ERR_INVALID on a malformed stream (the
 *                       reference's load returns false).  Host only, no GPU.
 * mbrwt_tree_serialize  BRWT::serialize (BRWT.cpp:113-128) of a description:
 *                       capacity protocol as mbrwt_get_rows (buf may be NULL
 *                       for the sizing call).  Host only, no GPU.
 * mbrwt_tree_export     the tree a context holds, read back from its device
 *                       image (every node's index column; any image layout).
 * mbrwt_load            mbrwt_tree_parse + mbrwt_create.
 */
typedef struct mbrwt_tree mbrwt_tree;
int mbrwt_tree_parse(const uint8_t *bytes, uint64_t len, uint64_t *consumed, mbrwt_tree **out);
int mbrwt_tree_serialize(const mbrwt_tree_desc *desc, uint8_t *buf, uint64_t cap, uint64_t *needed);
int mbrwt_tree_export(mbrwt_ctx *ctx, mbrwt_tree **out);
/* The shape BRWTBottomUpBuilder::build gives with get_basic_partitioner(arity)
   (BRWT_builders.cpp:20-31, :119-163; groups of one pass through, so leaves
   may sit at mixed depths): an owned mbrwt_tree with every vec_size 0 (and
   num_rows 0) -- the shape mbrwt_create_from_rows takes for shape == NULL.
   arity outside 2..64 -> MBRWT_ERR_INVALID; num_columns == 0 gives the empty
   tree.  Host only, no GPU. */
int mbrwt_tree_basic_shape(uint64_t num_columns, uint32_t arity, mbrwt_tree **out);

/* ---- tree shapes straight from row-major data ------------
 * The shape the reference's production build gives -- binary_grouping_greedy
 * (partitionings.cpp:148-196) then BRWTOptimizer::relax (BRWT_builders.cpp:
 * 166-297; `transform_anno --greedy`, `relax_brwt`) -- from the CSR of the
 * rows alone: no dense column and no index column is built anywhere.
 *
 * mbrwt_rows_node_counts: counts[u] (num_nodes u64, host) = the rows of desc
 * with a label below BFS node u of the shape (a leaf: its column's popcount;
 * the root: the non-empty rows).  shape == NULL: mbrwt_tree_basic_shape(
 * num_columns, arity).  One pass over all rows on the device, range by range
 * as mbrwt_create_from_rows ranges (multiples of 360,360 rows sized from the
 * free device memory, MBRWT_BUILD_ROWS_RANGE honoured); arguments, shape and
 * rows are checked as there, with the same statuses.  Limits
 * (MBRWT_ERR_UNSUPPORTED): more than 65,536 columns, a shape of height > 16,
 * a row of more than 32,767 labels.  A one-column shape is allowed.
 * num_rows == 0 or num_columns == 0: all-zero counts.
 *
 * mbrwt_tree_relax_shape: BRWTOptimizer::relax(max_arity) of `shape` given
 * such counts -- a node's index column has counts[parent] bits of which
 * counts[node] are set, and that is all relax's decisions read -- as an owned
 * shape-only tree (vec_size 0, num_rows 0), renumbered breadth-first.
 * max_arity <= 1: the shape unchanged.  Host only, no GPU.
 *
 * mbrwt_tree_shape_from_rows: partitioner MBRWT_PARTITIONER_BASIC (arity
 * 2..64) or MBRWT_PARTITIONER_GREEDY (arity ignored; the similarities over
 * the reference's row sample, gathered from the CSR), then, for
 * relax_max_arity > 1, the counts over ALL rows and the relax above: the
 * shape BRWTBottomUpBuilder::build + BRWTOptimizer::relax give on the dense
 * matrix of these rows, ready for mbrwt_create_from_rows.  Another
 * partitioner, or an arity outside 2..64 under BASIC -> MBRWT_ERR_INVALID.
 * The greedy partitioner checks the sampled rows' columns, the counts pass
 * those of every row; BASIC without relax reads no row.  The thread's
 * MBRWT_BUILD_PARTITIONER is not read. */
int mbrwt_rows_node_counts(const mbrwt_rows_desc *desc, const mbrwt_shape_desc *shape, uint32_t arity, int device,
                           uint64_t *counts);
int mbrwt_tree_relax_shape(const mbrwt_shape_desc *shape, const uint64_t *counts, uint64_t max_arity,
                           mbrwt_tree **out);
int mbrwt_tree_shape_from_rows(const mbrwt_rows_desc *desc, int partitioner, uint32_t arity,
                               uint64_t relax_max_arity, int device, mbrwt_tree **out);
/* The same two from sparse columns, with the arguments,
 * limits and statuses of mbrwt_create_from_sparse_columns:
 * mbrwt_sparse_columns_node_counts equals mbrwt_rows_node_counts of the same
 * matrix (the ranges transposed on the device, every id checked);
 * mbrwt_tree_shape_from_sparse_columns equals mbrwt_tree_shape_from_rows node
 * for node.  The greedy partitioner's sample (the reference's 10^6 sampled
 * rows; every row up to 10^6 rows) is intersected with every column's ids on
 * the host and scattered into the sample columns on the device; it checks the
 * ids when every row is sampled, the counts pass (relax_max_arity > 1)
 * always. */
int mbrwt_sparse_columns_node_counts(const mbrwt_sparse_columns_desc *desc, const mbrwt_shape_desc *shape,
                                     uint32_t arity, int device, uint64_t *counts);
int mbrwt_tree_shape_from_sparse_columns(const mbrwt_sparse_columns_desc *desc, int partitioner, uint32_t arity,
                                         uint64_t relax_max_arity, int device, mbrwt_tree **out);
const mbrwt_tree_desc *mbrwt_tree_get_desc(const mbrwt_tree *tree); /* valid until mbrwt_tree_free */
void mbrwt_tree_free(mbrwt_tree *tree);
int mbrwt_load(const uint8_t *bytes, uint64_t len, uint64_t *consumed, int device, mbrwt_ctx **out);

/* ---- properties (BRWT.hpp:33-51) -------------------------------------- */
uint64_t mbrwt_num_rows(const mbrwt_ctx *ctx);
uint64_t mbrwt_num_columns(const mbrwt_ctx *ctx);
uint64_t mbrwt_num_relations(const mbrwt_ctx *ctx);
uint64_t mbrwt_num_nodes(const mbrwt_ctx *ctx);
uint64_t mbrwt_device_bytes(const mbrwt_ctx *ctx); /* HBM held by the structure image */
int mbrwt_device(const mbrwt_ctx *ctx);
/*
 * Row shards: the reference's Row is uint64_t (binary_matrix.hpp:11).  One
 * device image addresses < 2^32 positions, so a context over more rows
 * (mbrwt_create, mbrwt_load, mbrwt_create_synthetic[_shaped]) holds row
 * shards of 2^31 rows -- each the BRWT restricted to its row range -- and
 * routes every query's rows to them; results are those of the whole matrix.
 * mbrwt_num_shards = 1 for an ordinary context.  (The build option
 * MBRWT_BUILD_SHARD_ROWS forces smaller shards: a test hook.)
 */
uint64_t mbrwt_num_shards(const mbrwt_ctx *ctx);

/* ---- queries ----------------------------------------------------------- */
/*
 * Batched BRWT::get_row over rows[0..n): CSR result with offsets[0..n]
 * (n+1 entries, offsets[0] = 0) and cols[offsets[i]..offsets[i+1]) = row i's
 * column ids in the reference's order.  If the total exceeds cols_cap,
 * returns MBRWT_ERR_CAPACITY with *cols_needed set to the total (retry
 * protocol); offsets and cols are then unspecified (a prefix of the CSR
 * may have been written).  cols_needed may be NULL.  Host buffers: the
 * batch is cut into chunks of 2^20 rows whose upload, query and download
 * overlap (r05, hostpipe.cpp); page-locked buffers (hipHostMalloc,
 * hipHostRegister) are read and written by DMA directly, pageable ones are
 * staged through the context's pinned buffers by a pool of host threads.
 */
int mbrwt_get_rows(mbrwt_ctx *ctx, const uint64_t *rows, uint64_t n, uint64_t *offsets, uint32_t *cols,
                   uint64_t cols_cap, uint64_t *cols_needed);

/*
 * Same on device buffers (d_rows: n uint64; d_offsets: n+1 uint64; d_cols:
 * cols_cap uint32), enqueued on HIP stream `stream` (hipStream_t, NULL =
 * default stream).  The call synchronises `stream` once to learn the output
 * size; the results are complete when `stream` is next synchronised.
 */
int mbrwt_get_rows_device(mbrwt_ctx *ctx, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets,
                          uint32_t *d_cols, uint64_t cols_cap, uint64_t *cols_needed, void *stream);

/*
 * The same without any host synchronisation, for pipelines that keep the
 * device busy (consecutive batches, the multi-GPU exchange): the call only
 * enqueues work on `stream`.  When the stream reaches its end, d_status
 * (device memory, 3 uint64) holds {labels needed, MBRWT_* status of the
 * call, sticky bits |= 1 << status} -- the caller clears word 2 and checks
 * it after synchronising.  Over cols_cap the status is MBRWT_ERR_CAPACITY
 * and no label is written past cols_cap (offsets may be); out-of-range rows give
 * MBRWT_ERR_RANGE.  The return value reports only argument and launch errors.
 * On a per-node image the call runs the synchronous path (one host sync)
 * and then writes the same status block.
 */
int mbrwt_get_rows_device_async(mbrwt_ctx *ctx, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets,
                                uint32_t *d_cols, uint64_t cols_cap, uint64_t *d_status, void *stream);

/*
 * The three calls above with 16-bit labels: cols / d_cols holds uint16_t and
 * cols_cap / cols_needed count uint16_t elements; offsets, label order, the
 * capacity protocol, the NULL-cols count-only call and the status block are
 * those of the u32 calls.  For contexts of at most 65,536 columns (exactly
 * 65,536 is allowed: label 65,535 is a value, not a sentinel); a context of
 * more answers MBRWT_ERR_UNSUPPORTED before any launch, with the column count
 * in mbrwt_last_error_message.  Alignment: d_cols must be aligned to 2 bytes,
 * nothing more (a slice at an odd element offset of a larger buffer is fine).
 * Row-record contexts store the narrow labels in their last kernel (half the
 * label bytes written, and half downloaded by the host call); every other
 * context (per-node images, row shards, a forced MBRWT_OPT_KERNEL variant)
 * runs its u32 query into a context workspace of 4 bytes per label and
 * narrows into the caller's buffer, so there the call costs the u32 call
 * plus one pass over the labels.
 */
int mbrwt_get_rows16(mbrwt_ctx *ctx, const uint64_t *rows, uint64_t n, uint64_t *offsets, uint16_t *cols,
                     uint64_t cols_cap, uint64_t *cols_needed);
int mbrwt_get_rows16_device(mbrwt_ctx *ctx, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets,
                            uint16_t *d_cols, uint64_t cols_cap, uint64_t *cols_needed, void *stream);
int mbrwt_get_rows16_device_async(mbrwt_ctx *ctx, const uint64_t *d_rows, uint64_t n, uint64_t *d_offsets,
                                  uint16_t *d_cols, uint64_t cols_cap, uint64_t *d_status, void *stream);

/* Batched BRWT::get (BRWT.cpp:9-24): out[i] = bit (rows[i], cols[i]). Host buffers. */
int mbrwt_get_batch(mbrwt_ctx *ctx, const uint64_t *rows, const uint64_t *cols, uint64_t n, uint8_t *out);
int mbrwt_get_batch_device(mbrwt_ctx *ctx, const uint64_t *d_rows, const uint64_t *d_cols, uint64_t n,
                           uint8_t *d_out, void *stream);

/*
 * BRWT::get_column (BRWT.cpp:55-85; BinaryMatrix::get_column,
 * binary_matrix.hpp:21): the ascending rows carrying `column`, written to
 * rows[0..*rows_needed).  If the column has more than rows_cap rows, returns
 * MBRWT_ERR_CAPACITY with *rows_needed set and rows untouched (call with
 * rows_cap = 0 to size the buffer).  column >= num_columns -> MBRWT_ERR_RANGE
 * (an assert in the reference).  Host buffer / device buffer + stream.
 */
int mbrwt_get_column(mbrwt_ctx *ctx, uint64_t column, uint64_t *rows, uint64_t rows_cap, uint64_t *rows_needed);
int mbrwt_get_column_device(mbrwt_ctx *ctx, uint64_t column, uint64_t *d_rows, uint64_t rows_cap,
                            uint64_t *rows_needed, void *stream);

/*
 * Batched column extraction: the sparse columns of the row window [row_begin,
 * row_end) for many columns at once -- the inverse of
 * mbrwt_create_from_sparse_columns (the reference's ColumnCompressed form,
 * ascending row ids per column).  The result is a CSR by REQUESTED SLOT:
 * rows[offsets[j] .. offsets[j + 1]) = the ascending absolute row ids r,
 * row_begin <= r < row_end, that carry columns[j], i.e.
 * mbrwt_get_column(columns[j]) clipped to the window; offsets[0] = 0, n_columns
 * + 1 offsets.  Slots come in the caller's order, which need not ascend.
 *   columns     a HOST array (in both forms, like `counts` of
 *               mbrwt_unpack_segments_device).  NULL = every column 0 ..
 *               num_columns - 1 in order; n_columns must then equal
 *               num_columns.  n_columns == 0 is legal: offsets[0] = 0,
 *               *rows_needed = 0, MBRWT_OK.
 *   capacity    a total above rows_cap, or rows == NULL with a non-zero total,
 *               returns MBRWT_ERR_CAPACITY: *rows_needed (may be NULL) holds
 *               the total, offsets is COMPLETE (the sizing call yields every
 *               column's size) and rows is untouched.
 *   errors      a column >= num_columns, row_begin > row_end or row_end >
 *               num_rows -> MBRWT_ERR_RANGE; a column listed twice ->
 *               MBRWT_ERR_INVALID (the message names it); NULL ctx or offsets
 *               -> MBRWT_ERR_INVALID, with or without a GPU; columns == NULL
 *               with n_columns neither 0 nor num_columns -> MBRWT_ERR_INVALID.
 *               All checked on the host before any launch.
 * On row records (layout ROWS, and BOTH through its records) the records are
 * swept twice whatever n_columns is -- a count sweep (it alone answers the
 * sizing call) and an emit sweep -- or three times when the window takes more
 * than one internal chunk (a chunk: at most 2^32 rows and 2^31 - 1 result
 * rows, sized from the free device memory: 16 bytes per result row of the
 * chunk -- 8 for a single column -- plus the sort's histograms, and 4 per row
 * of it).  Contexts without row records (layout NODES, row
 * shards) answer with mbrwt_get_column's work per column, twice.
 * Device form: the conventions of mbrwt_get_column_device (the context's
 * workspace fence; the results are complete on return); it synchronises
 * `stream` a bounded number of times per chunk, never per column, on row
 * records.  Host form: the result is staged in a context workspace (8 bytes
 * per returned row) and downloaded -- the window is how a caller bounds that.
 */
int mbrwt_get_columns(mbrwt_ctx *ctx, const uint64_t *columns, uint64_t n_columns, uint64_t row_begin,
                      uint64_t row_end, uint64_t *offsets, uint64_t *rows, uint64_t rows_cap, uint64_t *rows_needed);
int mbrwt_get_columns_device(mbrwt_ctx *ctx, const uint64_t *columns /* HOST, or NULL */, uint64_t n_columns,
                             uint64_t row_begin, uint64_t row_end, uint64_t *d_offsets /* n_columns + 1 */,
                             uint64_t *d_rows, uint64_t rows_cap, uint64_t *rows_needed, void *stream);

/*
 * StaticBinRelAnnotator::count_labels (annotate_static.cpp:149-162) fused on
 * the device: counts[c] (num_columns uint64, zeroed by the call) = number of
 * rows among d_rows[0..n) that carry column c.  Device buffers.
 */
int mbrwt_count_labels_device(mbrwt_ctx *ctx, const uint64_t *d_rows, uint64_t n, uint64_t *d_counts,
                              void *stream);

/*
 * StaticBinRelAnnotator::get_labels(indices, presence_ratio)
 * (annotate_static.cpp:71-94) for many reads at once -- the `classify`
 * consumer of get_rows.  Read r's row indices are
 * d_rows[d_read_offsets[r] .. d_read_offsets[r+1]) (n_reads + 1 ascending
 * offsets, the first 0, the last n_rows); its labels are the columns present
 * in at least ceil(len_r * presence_ratio) of its rows (in >= 1 row when the
 * ratio is 0), ascending.  Output: d_label_offsets[n_reads + 1] and d_labels
 * (capacity protocol as mbrwt_get_rows: MBRWT_ERR_CAPACITY + labels_needed).
 * presence_ratio outside [0, 1] (an assert in the reference) ->
 * MBRWT_ERR_INVALID; more than 15,360 columns -> MBRWT_ERR_UNSUPPORTED.
 * Device buffers + stream; mbrwt_get_labels_batch is the host-buffer form
 * (read_offsets validated as on the device: ascending, last = n_rows).
 */
int mbrwt_get_labels_batch(mbrwt_ctx *ctx, const uint64_t *rows, uint64_t n_rows, const uint64_t *read_offsets,
                           uint64_t n_reads, double presence_ratio, uint64_t *label_offsets, uint32_t *labels,
                           uint64_t labels_cap, uint64_t *labels_needed);
int mbrwt_get_labels_batch_device(mbrwt_ctx *ctx, const uint64_t *d_rows, uint64_t n_rows,
                                  const uint64_t *d_read_offsets, uint64_t n_reads, double presence_ratio,
                                  uint64_t *d_label_offsets, uint32_t *d_labels, uint64_t labels_cap,
                                  uint64_t *labels_needed, void *stream);

/*
 * MultiLabelEncoded::get_top_labels(indices, num_top) (annotate.cpp:57-83;
 * `classify --count-labels`, main.cpp:177) for many reads at once: read r's
 * labels present in >= 1 of its rows with their row counts, by count
 * descending, at most num_top of them.  Equal counts come in ascending label
 * order (the reference's std::sort leaves their order unspecified).  Reads as
 * mbrwt_get_labels_batch; output d_label_offsets[n_reads + 1], d_labels (u32)
 * and d_counts (u64) side by side, labels_cap entries each (capacity protocol
 * as mbrwt_get_rows).  More than 8,192 columns -> MBRWT_ERR_UNSUPPORTED.
 */
int mbrwt_get_top_labels_batch(mbrwt_ctx *ctx, const uint64_t *rows, uint64_t n_rows, const uint64_t *read_offsets,
                               uint64_t n_reads, uint64_t num_top, uint64_t *label_offsets, uint32_t *labels,
                               uint64_t *counts, uint64_t labels_cap, uint64_t *labels_needed);
int mbrwt_get_top_labels_batch_device(mbrwt_ctx *ctx, const uint64_t *d_rows, uint64_t n_rows,
                                      const uint64_t *d_read_offsets, uint64_t n_reads, uint64_t num_top,
                                      uint64_t *d_label_offsets, uint32_t *d_labels, uint64_t *d_counts,
                                      uint64_t labels_cap, uint64_t *labels_needed, void *stream);

/* ---- measurement ------------------------------------------------------- */
/*
 * Roofline accounting (DESIGN.md "Measurement"): over rows[0..n) (device
 * buffer) return sum V(row) (index-bit probes the reference recursion makes,
 * BRWT.cpp:30) and sum L(row) (labels returned).  Untimed diagnostic pass.
 */
int mbrwt_count_work_device(mbrwt_ctx *ctx, const uint64_t *d_rows, uint64_t n, uint64_t *sum_visits,
                            uint64_t *sum_labels, void *stream);

/* Options (mbrwt_set_option). */
/* ---- multi-GPU exchange helpers --------------------------------------- */
/*
 * Bit-packing of n values < 2^bits (bits in 1..32) into ceil(n*bits/32) u32
 * words (value i at bits [i*bits, (i+1)*bits), LSB-first), and back; device
 * buffers, launched on `stream`.  Only the low `bits` bits of a value (here,
 * and of a label or a row count in mbrwt_pack_csr_device) reach the wire: a
 * value with higher bits set is packed as its low bits and never disturbs a
 * neighbouring value.  The all-gatherv that reassembles a sharded
 * batch's CSR (genome_graph_annotation_amd/dist.py) ships labels and row
 * counts at ceil(log2(num_columns)) bits with these.  No reference
 * counterpart (the reference has no multi-GPU path).
 */
int mbrwt_pack_ids_device(const uint32_t *d_values, uint64_t n, uint32_t bits, uint32_t *d_words, void *stream);
int mbrwt_unpack_ids_device(const uint32_t *d_words, uint64_t n, uint32_t bits, uint32_t *d_values, void *stream);
/* The unpacking of a whole all-gathered wire buffer in one launch: segment r
   (r < nseg) starts at d_base + r * seg_stride bytes (a multiple of 4) and
   holds counts[r] (host array) packed values; they are written to d_values
   back to back in segment order. */
int mbrwt_unpack_segments_device(const void *d_base, uint32_t nseg, uint64_t seg_stride, const uint64_t *counts,
                                 uint32_t bits, uint32_t *d_values, void *stream);
/* The all-gatherv with DEVICE-side sizes (no host synchronisation per
   exchange; dist.py AllGatherV(device_sizes=True)).  A rank's wire segment of
   `wire_bytes` (a multiple of 16) is
     [u64 num_labels][n_rows row counts at bits_count][zero pad to 16 bytes]
     [min(num_labels, labels_cap) labels at bits_label][zero pad]
   with both fields in whole chunks of 32 values (a chunk = bits words;
   value i at bits [i*bits, (i+1)*bits) of the field, LSB-first)
   with num_labels read from the device (*d_num_labels, e.g. word 0 of the
   status block of mbrwt_get_rows_device_async) and the row counts taken
   from the CSR offsets (offsets[i+1] - offsets[i]); d_cols holds cols_cap
   labels: num_labels > cols_cap (the rank's get_rows failed on capacity, its
   CSR unwritten) writes the header 2^64 - 1 and nothing else, so the unpack
   flags the exchange; the label field starts
   at byte labels_offset (a multiple of 16, at least
   mbrwt_wire_labels_offset(n_rows, bits_count): every rank of an exchange
   uses the offset of the largest slice) and needs
   ceil(labels_cap / 32) * bits_label words.
   MBRWT_ERR_INVALID when the layout does not fit wire_bytes. */
uint64_t mbrwt_wire_labels_offset(uint64_t n_rows, uint32_t bits_count);
int mbrwt_pack_csr_device(const uint64_t *d_offsets, uint64_t n_rows, const uint32_t *d_cols, uint64_t cols_cap,
                          const uint64_t *d_num_labels, uint64_t labels_cap, uint32_t bits_count, uint32_t bits_label,
                          uint64_t labels_offset, void *d_wire, uint64_t wire_bytes, void *stream);
/* The labels of every segment of an all-gathered buffer of such segments
   (segment r at d_base + r * seg_stride; its label field at labels_offset
   bytes), written back to back in segment order: the segments' label counts
   and their prefix are read from the headers ON THE DEVICE.  d_status[0] =
   the total, d_status[1] = 0, or 1 when a header exceeds labels_cap or the
   total exceeds values_cap (nothing is written then). */
int mbrwt_unpack_labels_device(const void *d_base, uint32_t nseg, uint64_t seg_stride, uint64_t labels_offset,
                               uint64_t labels_cap, uint32_t bits, uint32_t *d_values, uint64_t values_cap,
                               uint64_t *d_status, void *stream);

/* The global CSR offsets of an all-gathered wire straight from its packed
   row counts (r04): d_offsets[0 .. N] = the exclusive prefix of every
   segment's counts (segment r: counts[r] values of `bits` bits each at byte
   8 of d_base + r * seg_stride, the layout mbrwt_pack_csr_device writes),
   N = sum(counts) -- block sums, one workgroup's scan of them, then every
   block's counts re-read and scanned in LDS (no int32 count array in
   between).  d_temp == NULL: *temp_bytes receives the
   scratch size the call needs and nothing runs.  At most 8 segments (one
   node); MBRWT_ERR_UNSUPPORTED beyond (unpack the counts and scan them). */
int mbrwt_unpack_offsets_device(const void *d_base, uint32_t nseg, uint64_t seg_stride, const uint64_t *counts,
                                uint32_t bits, uint64_t *d_offsets, void *d_temp, uint64_t *temp_bytes,
                                void *stream);

#define MBRWT_OPT_TIMING 1       /* 1: time the traversal kernel with HIP events */
#define MBRWT_OPT_SLOT_LABELS 2  /* per-row label slots of the fast path (0 = auto) */
#define MBRWT_OPT_KERNEL 4       /* traversal kernel: 0 the default (the row-record kernels; on node images
                                    k_traverse_ptw / k_traverse_p2w / k_traverse_fast2 where the tree is
                                    eligible, else the group kernel), 1 the lane-per-row node-image kernel
                                    (A/B and tests; needs layout NODES or BOTH, else MBRWT_ERR_UNSUPPORTED).
                                    The retired A/B variants 2..6, 10, 17..20 and 24..30 return
                                    MBRWT_ERR_UNSUPPORTED (what they measured: profiles/r02 .. r04), any
                                    other value MBRWT_ERR_INVALID. */
#define MBRWT_OPT_ROWS_WALK 8  /* row records: 0 default (the odometer walk over the path table on uniform
                                   trees, the tree odometer on every other shape of <= 8 internal levels),
                                   3 the tree odometer, 4 the stack walk, 6 the stack walk of one-byte masks,
                                   7 the odometer without the path table (A/B and tests) */
#define MBRWT_OPT_COMPACT_CUS 64 /* row records (r06, measurement): 0 default; k in 1..31 runs the
                                    compaction of get_rows_device on a stream masked to k of every 32 CUs
                                    (hipExtStreamCreateWithCUMask), after the traversal and before the
                                    caller's stream by two events */
#define MBRWT_OPT_TEST_FAIL_CHUNK 32 /* test hook: mbrwt_get_rows (host buffers) fails with MBRWT_ERR_NOMEM
                                        when it reaches chunk `value` of the batch (-1: never) -- the error
                                        path's drain of the chunks already in flight is tested with it */
#define MBRWT_OPT_COLUMNS_CHUNK 128 /* test hook: rows per internal chunk of mbrwt_get_columns* on row records
                                       (0 = auto, from the free device memory) -- the chunk cursors are tested
                                       with it at small shapes */
int mbrwt_set_option(mbrwt_ctx *ctx, int option, int64_t value);

/* Traversal-kernel time accumulated while MBRWT_OPT_TIMING is on (ms, launches); resets the sums. */
int mbrwt_take_timing(mbrwt_ctx *ctx, double *kernel_ms, uint64_t *launches);

const char *mbrwt_strerror(int status);
const char *mbrwt_last_error_message(void); /* thread-local detail of the last failure */

/* Diagnostics: name of the traversal kernel mbrwt_get_rows* launches for this
   tree under the current MBRWT_OPT_KERNEL (static string; "" for a null ctx). */
const char *mbrwt_traverse_kernel(mbrwt_ctx *ctx);

/* Diagnostics: the rows that the last mbrwt_get_rows*_device* call on the
   per-node images (one batch, no row shards) left to its direct pass -- rows
   of more labels than their slot, or the 16 rows of a rowblock of more labels
   than its 16 slots (MBRWT_OPT_SLOT_LABELS).  0 for a null ctx. */
uint64_t mbrwt_overflow_rows(mbrwt_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* MBRWT_H */
