// Pipeline::find_entities_in_boxes of the C++ host mirror (include/render_engine_hip.hpp): the tree query the logic callbacks get instead of
// &BoundingBoxTree, on a handful of instances: before the first frame (the query uploads the world), with a filter, after an instance was added
// between frames, and with a box that touches an instance exactly on its face.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "render_engine_hip.hpp"

using namespace render_engine;

static int fail(const char *what) { std::printf("FAIL: %s\n", what); return 1; }

using Pair = std::pair<uint32_t, uint32_t>;
static std::vector<Pair> sorted(const std::vector<re_box_hit> &hits) {
    std::vector<Pair> out;
    for (const re_box_hit &h : hits) out.emplace_back(h.query, h.entity_id);
    std::sort(out.begin(), out.end());
    return out;
}
static StaticAABB cube(float x, float y, float z, float half) { return StaticAABB{ { x - half, x + half }, { y - half, y + half }, { z - half, z + half } }; }

int main() {
    Camera camera = CameraBuilder({ 1280, 720 }).with_position(vec3(1000.0f, 1000.0f, 1150.0f)).with_direction(vec3(0.0f, 0.0f, -1.0f)).with_far_draw_distance(1000.0f).build();
    Pipeline pipeline(16384, 64);
    const StaticAABB box{ { -1.0f, 1.0f }, { -1.0f, 1.0f }, { -1.0f, 1.0f } };
    std::vector<EntityId> made;
    auto place = [&](float x, float z, bool is_static) {
        pipeline.register_model_instances(ModelId{ 2, 0 }, 1, box, [&](Pipeline &p, const std::vector<EntityId> &created, StaticAABB aabb) {
            EntityTransformationBuilder b(created[0], is_static, std::nullopt, false);
            b.with_translation(Position::new_(vec3(x, 1000.0f, z)));
            b.apply_choices(aabb, p);
            made.push_back(created[0]);
        });
    };
    place(970.0f, 1000.0f, false); place(1023.0f, 1000.0f, false); place(1025.0f, 1000.0f, true);      // [1022, 1024]: its maximum lies on the section border x = 1024
    const EntityId a = made[0], b = made[1], c = made[2];
    // box 0 around a; box 1 from x = 1024 on: touches b on its face and covers c; box 2: nobody
    const std::vector<StaticAABB> boxes{ cube(970.0f, 1000.0f, 1000.0f, 10.0f), StaticAABB{ { 1024.0f, 1030.0f }, { 990.0f, 1010.0f }, { 990.0f, 1010.0f } }, cube(500.0f, 500.0f, 500.0f, 20.0f) };
    const std::vector<Pair> want{ Pair{ 0u, a }, Pair{ 1u, b }, Pair{ 1u, c } };
    if (sorted(pipeline.find_entities_in_boxes(boxes)) != want) return fail("pairs before the first frame");
    if (sorted(pipeline.find_entities_in_boxes(boxes, 0u, RE_F_STATIC)) != std::vector<Pair>{ Pair{ 0u, a }, Pair{ 1u, b } }) return fail("forbid RE_F_STATIC");
    if (sorted(pipeline.find_entities_in_boxes(boxes, RE_F_STATIC)) != std::vector<Pair>{ Pair{ 1u, c } }) return fail("need RE_F_STATIC");
    pipeline.execute(camera, 1.0f / 60.0f);
    place(975.0f, 1005.0f, false);                                     // registered after frames have run: appended
    const EntityId late = made[3];
    std::vector<Pair> want2 = want; want2.push_back(Pair{ 0u, late }); std::sort(want2.begin(), want2.end());
    if (sorted(pipeline.find_entities_in_boxes(boxes)) != want2) return fail("pairs with an instance added later");
    if (!pipeline.find_entities_in_boxes({}).empty()) return fail("no boxes, no pairs");
    try { pipeline.find_entities_in_boxes({ StaticAABB{ { 2.0f, 1.0f }, { 0.0f, 1.0f }, { 0.0f, 1.0f } } }); return fail("an inverted box is refused"); }
    catch (const Error &e) { if (e.code != RE_E_ARG) return fail("an inverted box is RE_E_ARG"); }
    std::printf("OK box queries through the C++ mirror\n");
    return 0;
}
